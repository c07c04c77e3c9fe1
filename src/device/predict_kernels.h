// Prediction from raw feature rows on the device (Booster.predict_device): the launch plan of
// k_predict_raw / k_predict_leaf. The plan is plain host arithmetic, kept apart from the
// kernels so its thresholds are stated once.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "device/predict_pack.h"

namespace lgap {
namespace device {

constexpr int kPThreads = 256;
constexpr int kPRowsPerThread = 2;                        // independent walks per lane
constexpr int kPTileRows = kPThreads * kPRowsPerThread;   // rows of one block pass
constexpr int kPTreeLdsBytes = 8 * 1024;                  // staged trees: nodes + leaf values
constexpr int kPTileLdsBytes = 56 * 1024;                 // staged rows + LDS accumulators
constexpr int kPRegClasses = 4;                           // accumulators per row kept in registers

// LDS bytes of `nodes` nodes and `leaves` leaf values staged together (leaf values 16-byte aligned)
inline size_t PredictTreeLdsBytes(size_t nodes, size_t leaves) {
  return ((nodes * sizeof(PNode) + 15) & ~static_cast<size_t>(15)) + leaves * sizeof(double);
}

// A run of consecutive trees whose nodes and leaf values are staged in LDS together, or one
// tree too large for that, walked from global memory (staged = 0).
struct PredictBatch {
  int32_t first, count;
  int32_t node_begin, node_count;
  int32_t leaf_begin, leaf_count;
  int32_t staged, pad;
};
std::vector<PredictBatch> PlanPredictBatches(const PackedEnsemble& pk);

struct PredictShape {
  int tile_rows;    // rows per block pass (<= kPTileRows)
  int stage_rows;   // the tile's rows are staged in LDS
  int acc_lds;      // accumulators in LDS (more than kPRegClasses trees per iteration)
  size_t lds_bytes; // dynamic LDS of the launch
};
// leaf: k_predict_leaf (no accumulators); elem: bytes of one feature value
PredictShape PlanPredictShape(int ncol, size_t elem, int num_tree_per_iteration, bool leaf);

// ---- the tree-parallel path of the resident predictor (k_predict_pairs, then k_predict_fold):
// a block owns one PredictBatch and a tile of rows, its lanes spread over the (row, tree) pairs.
constexpr int kPairSmallTileRows = 64;            // the row tile of batches up to kPairSmallTileMaxRows
constexpr int kPairLargeTileRows = 256;           // and of larger ones: each staged run serves more rows
constexpr int kPairSmallTileMaxRows = 1024;
constexpr int kPairRowLdsBytes = 32 * 1024;       // a tile's rows are staged in LDS up to this size
constexpr int kTreeParallelMaxRows = 65536;       // bounds the [tree][row] scratch
// Batches of at most this many rows take the tree-parallel path unless the caller says otherwise.
// Measured (profiles/device_predictor.md): faster than the row-parallel kernels at every row
// count of the grid up to the limit.
constexpr int kTreeParallelDefaultRows = kTreeParallelMaxRows;

struct PairShape {
  int tile_rows;     // rows per block
  int stage_rows;    // the tile's rows are staged in LDS
  size_t lds_bytes;  // dynamic LDS of the launch
  long long grid;    // row tiles x batches, one block each
};
PairShape PlanPairShape(int nrow, int ncol, size_t elem, int num_batches);

}  // namespace device
}  // namespace lgap
