// Host-callable entry points of the HIP device layer (src/device/*.hip).
// Kept free of HIP headers so plain C++ translation units can include it.
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "lgap/config.h"
#include "lgap/split_math.h"
#include "lgap/tree_learner.h"

namespace lgap {
struct StridedChunk;  // lgap/dataset.h
namespace device {

// Number of visible MI355X (gfx950) devices; 0 when no GPU / no driver.
int DeviceCount();
// hipDeviceSynchronize on the current device (no-op without a GPU).
void DeviceSynchronize();
// Total memory of the current device in bytes (0 without a GPU).
size_t DeviceTotalMemory();
// RCCL communicator over xGMI for the multi-GPU learners.
std::string CommGetUniqueId();
void CommInit(const std::string& unique_id, int num_ranks, int rank, int device_id);
void CommFree();
int CommRank();
int CommSize();
bool CommActive();

// Single-process HIP tree learner (device_type=gpu|cuda) and its data-parallel
// variant (tree_learner=data|voting|feature with an RCCL communicator).
// TreeLearner::Create routes here what the engine plan (src/device/engine_plan.h) serves on the device.
std::unique_ptr<TreeLearner> CreateDeviceTreeLearner(const Config* config, const std::string& parallel_mode);

// GPU histogram engine for the host learners (the reference's GPUTreeLearner
// split, src/treelearner/gpu_tree_learner.cpp: histograms on the device, split
// policy on the host). Used when a host-side policy (CEGB, forced splits,
// intermediate/advanced monotone, linear leaves, voting/feature parallel) is
// requested with device_type=gpu. Gradients are uploaded once per tree.
class HistogramBackend {
 public:
  virtual ~HistogramBackend() = default;
  virtual void SetGradients(const float* grad, const float* hess, int num_data) = 0;
  // out: 2 * num_total_bin doubles (group bin 0 left zero, as the host builder)
  virtual void Histogram(const int* rows, int num_rows, double* out) = 0;
  virtual std::string DeviceName() const = 0;

  // ---- device-resident histograms and device split scans (intermediate / advanced monotone
  // constraints: src/device/policy_scan.h). The host keeps only the tree, the row partition and
  // the constraint bookkeeping; histograms never leave the device, scans return SplitInfo rows.
  // Allocates `num_slots` histogram slots of 2 * num_total_bin doubles; false: not available.
  virtual bool EnableResidentSlots(int num_slots) { (void)num_slots; return false; }
  // slot <- histogram of `rows` (all rows when null)
  virtual void HistogramToSlot(const int* rows, int num_rows, int slot) { (void)rows; (void)num_rows; (void)slot; }
  // larger <- larger - smaller (the parent's histogram held by the larger child's slot)
  virtual void SubtractSlots(int larger, int smaller) { (void)larger; (void)smaller; }
  // Scans the batch's leaves over every feature. Per leaf r: slot, row count, sums, parent output;
  // per (r, f): enable flag, flat bounds and (advanced) the offset of lmin / lmax / rmin / rmax
  // (num_bin doubles each) in `tb`, or -1. Returns out[r * F + f] (feature -1 when the feature
  // cannot split) and splittable[r * F + f].
  struct ScanBatch {
    std::vector<int> slot, count;
    std::vector<double> sum_g, sum_h, parent_output;
    std::vector<uint8_t> enable;
    std::vector<double> bmin, bmax;
    std::vector<long long> tb_off;
    std::vector<double> tb;
    void Clear() {
      slot.clear(); count.clear(); sum_g.clear(); sum_h.clear(); parent_output.clear();
      enable.clear(); bmin.clear(); bmax.clear(); tb_off.clear(); tb.clear();
    }
  };
  virtual void ScanSlots(const ScanBatch& batch, const SplitParams& params, SplitInfo* out, uint8_t* splittable) {
    (void)batch; (void)params; (void)out; (void)splittable;
  }
};
std::unique_ptr<HistogramBackend> CreateHistogramBackend(const Config* config, const Dataset* data);

// Histogram of (grad, hess) over `rows` (all rows when null) with the HIP
// histogram kernel; out has 2 * num_total_bin doubles.
void DeviceHistogram(const Dataset* data, const float* grad, const float* hess, const int* rows, int num_rows,
                     double* out);

// Direct tests of the frontier's production kernels (tests/test_frontier_kernels.py):
// k_f_hist over k row subsets (rows concatenated, offsets[k + 1]) -> out[k][num_total_bin][2]
// at the kernel's fixed-point scale (quantized training: integer level sums; levels[N] the
// quantized g << 8 | h levels); k_f_partition of k parents split by (inner feature, threshold
// bin / categorical bin set, default_left) -> the device's children lists and left counts, and
// the host learner's stable partition of the same split.
void TestFrontierHist(const Dataset* data, const Config& config, const float* grad, const float* hess, const int* rows,
                      const int* offsets, int k, double* out, uint16_t* levels);
// k_f_scan of the root round over all rows -> out[F][8] (gain, threshold, left count, default_left,
// left sum g, left sum h, valid, categorical thresholds), ref[F][8] the host split_math.h scan
void TestFrontierScan(const Dataset* data, const Config& config, const float* grad, const float* hess, double* out,
                      double* ref);
void TestFrontierPartition(const Dataset* data, const Config& config, const int* rows, const int* offsets, int k,
                           const int* feats, const int* thr, const int* dleft, const uint32_t* catbits, int* out_rows,
                           int* out_left, int* exp_rows, int* exp_left);

// Direct test of the gradient quantizer (tests/test_quantize_kernels.py): a device learner of
// `config` (Init with const_hess), class-major grad / hess [num_class][N] uploaded afresh every
// round, then the learner's own QuantizeGradients(class) for every class, `rounds` times (k_qmax
// and k_quantize with its grid, seed and round counter). Per (round, class): out_gh[N][2] the
// de-quantized (g, h), out_levels[N] the packed int8 g << 8 | uint8 h levels (written only when
// the function returns true: integer-level histograms, bins <= 254), out_qmax[2] the bits of
// max |g| and max |h|, out_true[N][2] the kept inputs (quant_train_renew_leaf only).
bool TestQuantize(const Dataset* data, const Config& config, bool const_hess, const float* grad, const float* hess,
                  int num_class, int rounds, float* out_gh, uint16_t* out_levels, uint32_t* out_qmax,
                  float* out_true);
// Direct test of the forest traversal (tests/test_traverse_forest_kernel.py): a device learner of
// `config` on `data` with `score` [N] as its one-class training score; copies of the trees scaled
// by Tree::Shrinkage(scales[i]) are added in list order by one k_traverse_forest launch (grid_cap
// > 0 caps its grid), or with per_tree by one single-tree traversal each -> out[N]. info (may be
// null): {group-bin width of the rows read (0 = 4-bit rows, 1, 2 bytes), dwords per row}.
void TestForestScore(const Dataset* data, const Config& config, const Tree* const* trees, const double* scales,
                     int count, const double* score, int grid_cap, bool per_tree, double* out, int* info);
// Direct test of the blended score update (tests/test_blend_score_kernel.py): a device learner of
// `config` on `data` with `score` [N] as its one-class training score; `tree` is blended in by the
// traversal route of DeviceBlendTreeIntoScore (a one-leaf tree: the blended constant): out[i] =
// divide ? (score[i] * pre + tree(i)) / post : (score[i] * pre + tree(i)) * post. grid_cap > 0 caps
// the kernel's grid.
void TestBlendScore(const Dataset* data, const Config& config, const Tree* tree, const double* score, double pre,
                    double post, bool divide, int grid_cap, double* out);
// Direct test of the linear-leaf Gram kernels (tests/test_linear_gram_kernel.py), no Dataset:
// raw[N][F], grad / hess[N]; leaf l reads segs[3 l ..] = (buffer, start, count): buffer 0 the
// positions [start, start + count) of rows[num_rows], buffer -1 the rows start .. start + count
// themselves; its features feats[feat_off[l] .. feat_off[l + 1]). One LaunchLinearGram with
// `chunks` row chunks per leaf -> out[num_leaves][64][64], usable[num_leaves].
void TestLinearGram(const float* raw, int N, int F, const float* grad, const float* hess, const int* rows,
                    int num_rows, const int* segs, int num_leaves, const int* feat_off, const int* feats,
                    int chunks, double* out, long long* usable);

// One pass of the device row-sampling kernels over host arrays (LGBM_DeviceSampleRows):
// returns the kept-row count, rows in out_rows, GOSS scaling applied to grad / hess.
int SampleRowsOnDevice(int mode, int num_rows, int num_class, float* grad, float* hess, const float* label,
                       double fraction, double pos_fraction, double neg_fraction, double top_rate, double other_rate,
                       int bagging_seed, uint32_t goss_seed, int rounds, int* out_rows);
// The same kernels for a direct test (LGBM_DeviceTestSampleRows, tests/test_sample_kernels.py): also
// mode 4, bagging by query, with row_unit / num_units built from query_sizes[num_queries] and
// LaunchSampleAdvanceUnits after every round as the learner launches it; with_oob allocates the
// out-of-bag list. out_rows and out_oob (both [num_rows]) are filled with -1 before every round and
// returned whole, so writes past the counts show.
int TestSampleRows(int mode, int num_rows, int num_class, float* grad, float* hess, const float* label,
                   const int* query_sizes, int num_queries, double fraction, double pos_fraction, double neg_fraction,
                   double top_rate, double other_rate, int bagging_seed, uint32_t goss_seed, int rounds, bool with_oob,
                   int* out_rows, int* out_oob);

// Feature binning on the device (bin_kernels.hip): packs `nrow` rows of a dense row-major
// matrix (fp32 / fp64) into `ds`'s packed group-bin layout (its mappers and EFB groups),
// writing host_out (nrow x row_stride bytes). With keep_device_copy the device rows stay
// registered for the HIP learner of `ds` (TakeDeviceRows). False: not supported here (the
// caller bins on the host).
bool DevicePackDense(const Dataset& ds, const void* data, bool f64, int nrow, int ncol, uint8_t* host_out,
                     bool keep_device_copy);
// The same for a matrix that already lives on the GPU (LGBM_DatasetCreateFromDeviceMats): row
// chunks read in place through element strides, no staging buffers and no upload. A contiguous
// row-major chunk runs k_pack_tiles / k_pack_rows as above; any other strides run
// k_pack_strided, which stages the same row tile with lanes along the unit stride. False with
// a reason in *why_not: the caller copies the matrix to the host. Fails without a GPU or for
// pointers that are not memory of the current device.
bool DevicePackResident(const Dataset& ds, const StridedChunk* chunks, int nchunk, bool f64, int ncol,
                        uint8_t* host_out, bool keep_device_copy, std::string* why_not);
// k_gather_rows: rows[0 .. n) (global row numbers over the chunks; null: rows first_row ..
// first_row + n) of device-resident chunks as a contiguous row-major [n x ncol] matrix of the
// chunks' dtype in host memory.
void GatherDeviceRows(const StridedChunk* chunks, int nchunk, bool f64, int ncol, const int* rows,
                      long long first_row, long long n, void* host_out);
// the device copy of `ds`'s packed rows (ownership moves to the caller; hipFree), or nullptr
// when none matches `bytes`
void* TakeDeviceRows(const Dataset* ds, size_t bytes);
void ReleaseDeviceRows(const Dataset* ds);

// Prediction from raw feature rows on the device (predict_kernels.hip). `pk` is the packed
// ensemble of src/device/predict_pack.h; mode is its kPredictRaw / kPredictLeaf. `data` holds
// nrow x ncol row-major fp32 / fp64 values, `out` nrow x (trees per iteration | trees) doubles;
// either may be host memory (moved in chunks of at most 256 MiB) or device memory, used in
// place. With device output a non-null transform is applied to the raw scores on the device
// (k_predict_convert). The work is complete when the call returns. Fails without a GPU.
struct PackedEnsemble;
enum PredictTransformKind : int { kTransformIdentity = 0, kTransformPointwise, kTransformSoftmax, kTransformOVA };
struct PredictTransform {
  int kind = kTransformIdentity;
  int output = 0;        // kTransformPointwise: PwOutput code (lgap/pointwise_metric.h)
  double sigmoid = 1.0;  // kOutSigmoid / kTransformOVA
};
void PredictDense(const PackedEnsemble& pk, const void* data, bool f64, int nrow, int ncol, int mode,
                  const PredictTransform* transform, bool data_on_device, bool out_on_device, double* out);

// A packed ensemble kept on the device for repeated prediction (Booster.device_predictor). The
// constructor uploads `pk` and its batch plan once; Predict takes PredictDense's arguments and
// gives its results. The object owns one non-blocking stream, device input / output buffers, the
// [tree][row] scratch of the tree-parallel kernels and, with `pinned`, pinned host staging
// buffers; all of them only grow, so a call whose shapes have been seen allocates nothing.
// Batches of at most tree_parallel_rows rows (0: none, at most 65,536) run k_predict_pairs and
// k_predict_fold, larger ones the row-parallel kernels. Calls are not serialised here.
enum PredictPath : int { kPathNone = -1, kPathRow = 0, kPathTree = 1 };
class ResidentEnsemble {
 public:
  ResidentEnsemble(const PackedEnsemble& pk, int tree_parallel_rows, bool pinned);
  ~ResidentEnsemble();
  ResidentEnsemble(const ResidentEnsemble&) = delete;
  ResidentEnsemble& operator=(const ResidentEnsemble&) = delete;
  void Predict(const void* data, bool f64, int nrow, int ncol, int mode, const PredictTransform* transform,
               bool data_on_device, bool out_on_device, double* out);
  int last_path() const { return last_path_; }  // the kernel family of the last call that launched

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
  int last_path_ = kPathNone;
};

}  // namespace device
}  // namespace lgap
