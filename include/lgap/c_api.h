/* LGBM_* compatible C ABI of LambdaGap-MI355X (reference: include/LightGBM/c_api.h).
 * Every function returns 0 on success and -1 on failure; LGBM_GetLastError()
 * returns the message. Handles are opaque pointers. */
#ifndef LGAP_C_API_H_
#define LGAP_C_API_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
#define LGAP_EXTERN_C extern "C"
#else
#define LGAP_EXTERN_C
#endif
#define LIGHTGBM_C_EXPORT LGAP_EXTERN_C __attribute__((visibility("default")))

typedef void* DatasetHandle;
typedef void* BoosterHandle;
typedef void* FastConfigHandle;
typedef void* DevicePredictorHandle;

#define C_API_DTYPE_FLOAT32 (0)
#define C_API_DTYPE_FLOAT64 (1)
#define C_API_DTYPE_INT32 (2)
#define C_API_DTYPE_INT64 (3)

#define C_API_PREDICT_NORMAL (0)
#define C_API_PREDICT_RAW_SCORE (1)
#define C_API_PREDICT_LEAF_INDEX (2)
#define C_API_PREDICT_CONTRIB (3)

#define C_API_FEATURE_IMPORTANCE_SPLIT (0)
#define C_API_FEATURE_IMPORTANCE_GAIN (1)

LIGHTGBM_C_EXPORT const char* LGBM_GetLastError();
LIGHTGBM_C_EXPORT int LGBM_RegisterLogCallback(void (*callback)(const char*));
LIGHTGBM_C_EXPORT int LGBM_DumpParamAliases(int64_t buffer_len, int64_t* out_len, char* out_str);
LIGHTGBM_C_EXPORT int LGBM_GetSampleCount(int32_t num_total_row, const char* parameters, int* out);
LIGHTGBM_C_EXPORT int LGBM_SampleIndices(int32_t num_total_row, const char* parameters, void* out, int32_t* out_len);

/* ---- Dataset */
LIGHTGBM_C_EXPORT int LGBM_DatasetCreateFromFile(const char* filename, const char* parameters,
                                                 const DatasetHandle reference, DatasetHandle* out);
LIGHTGBM_C_EXPORT int LGBM_DatasetCreateFromMat(const void* data, int data_type, int32_t nrow, int32_t ncol,
                                                int is_row_major, const char* parameters,
                                                const DatasetHandle reference, DatasetHandle* out);
LIGHTGBM_C_EXPORT int LGBM_DatasetCreateFromMats(int32_t nmat, const void** data, int data_type, int32_t* nrow,
                                                 int32_t ncol, int is_row_major, const char* parameters,
                                                 const DatasetHandle reference, DatasetHandle* out);
LIGHTGBM_C_EXPORT int LGBM_DatasetCreateFromCSR(const void* indptr, int indptr_type, const int32_t* indices,
                                                const void* data, int data_type, int64_t nindptr, int64_t nelem,
                                                int64_t num_col, const char* parameters,
                                                const DatasetHandle reference, DatasetHandle* out);
LIGHTGBM_C_EXPORT int LGBM_DatasetCreateFromCSC(const void* col_ptr, int col_ptr_type, const int32_t* indices,
                                                const void* data, int data_type, int64_t ncol_ptr, int64_t nelem,
                                                int64_t num_row, const char* parameters,
                                                const DatasetHandle reference, DatasetHandle* out);
LIGHTGBM_C_EXPORT int LGBM_DatasetCreateByReference(const DatasetHandle reference, int64_t num_total_row,
                                                    DatasetHandle* out);
LIGHTGBM_C_EXPORT int LGBM_DatasetInitStreaming(DatasetHandle dataset, int32_t has_weights, int32_t has_init_scores,
                                                int32_t has_queries, int32_t nclasses, int32_t nthreads,
                                                int32_t omp_max_threads);
LIGHTGBM_C_EXPORT int LGBM_DatasetPushRows(DatasetHandle dataset, const void* data, int data_type, int32_t nrow,
                                           int32_t ncol, int32_t start_row);
LIGHTGBM_C_EXPORT int LGBM_DatasetPushRowsWithMetadata(DatasetHandle dataset, const void* data, int data_type,
                                                       int32_t nrow, int32_t ncol, int32_t start_row,
                                                       const float* label, const float* weight,
                                                       const double* init_score, const int32_t* query, int32_t tid);
LIGHTGBM_C_EXPORT int LGBM_DatasetPushRowsByCSR(DatasetHandle dataset, const void* indptr, int indptr_type,
                                                const int32_t* indices, const void* data, int data_type,
                                                int64_t nindptr, int64_t nelem, int64_t num_col, int64_t start_row);
LIGHTGBM_C_EXPORT int LGBM_DatasetSetWaitForManualFinish(DatasetHandle dataset, int wait);
LIGHTGBM_C_EXPORT int LGBM_DatasetMarkFinished(DatasetHandle dataset);
LIGHTGBM_C_EXPORT int LGBM_DatasetGetSubset(const DatasetHandle handle, const int32_t* used_row_indices,
                                            int32_t num_used_row_indices, const char* parameters, DatasetHandle* out);
LIGHTGBM_C_EXPORT int LGBM_DatasetSetFeatureNames(DatasetHandle handle, const char** feature_names,
                                                  int num_feature_names);
LIGHTGBM_C_EXPORT int LGBM_DatasetGetFeatureNames(DatasetHandle handle, const int len, int* num_feature_names,
                                                  const size_t buffer_len, size_t* out_buffer_len,
                                                  char** feature_names);
LIGHTGBM_C_EXPORT int LGBM_DatasetFree(DatasetHandle handle);
LIGHTGBM_C_EXPORT int LGBM_DatasetSaveBinary(DatasetHandle handle, const char* filename);
LIGHTGBM_C_EXPORT int LGBM_DatasetDumpText(DatasetHandle handle, const char* filename);
LIGHTGBM_C_EXPORT int LGBM_DatasetSetField(DatasetHandle handle, const char* field_name, const void* field_data,
                                           int num_element, int type);
LIGHTGBM_C_EXPORT int LGBM_DatasetGetField(DatasetHandle handle, const char* field_name, int* out_len,
                                           const void** out_ptr, int* out_type);
LIGHTGBM_C_EXPORT int LGBM_DatasetUpdateParamChecking(const char* old_parameters, const char* new_parameters);
LIGHTGBM_C_EXPORT int LGBM_DatasetGetNumData(DatasetHandle handle, int* out);
LIGHTGBM_C_EXPORT int LGBM_DatasetGetNumFeature(DatasetHandle handle, int* out);
LIGHTGBM_C_EXPORT int LGBM_DatasetGetFeatureNumBin(DatasetHandle handle, int feature, int* out);
LIGHTGBM_C_EXPORT int LGBM_DatasetAddFeaturesFrom(DatasetHandle target, DatasetHandle source);

/* ---- Booster */
LIGHTGBM_C_EXPORT int LGBM_BoosterCreate(const DatasetHandle train_data, const char* parameters, BoosterHandle* out);
LIGHTGBM_C_EXPORT int LGBM_BoosterCreateFromModelfile(const char* filename, int* out_num_iterations,
                                                      BoosterHandle* out);
LIGHTGBM_C_EXPORT int LGBM_BoosterLoadModelFromString(const char* model_str, int* out_num_iterations,
                                                      BoosterHandle* out);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetLoadedParam(BoosterHandle handle, int64_t buffer_len, int64_t* out_len,
                                                 char* out_str);
LIGHTGBM_C_EXPORT int LGBM_BoosterFree(BoosterHandle handle);
LIGHTGBM_C_EXPORT int LGBM_BoosterShuffleModels(BoosterHandle handle, int start_iter, int end_iter);
LIGHTGBM_C_EXPORT int LGBM_BoosterMerge(BoosterHandle handle, BoosterHandle other_handle);
LIGHTGBM_C_EXPORT int LGBM_BoosterAddValidData(BoosterHandle handle, const DatasetHandle valid_data);
LIGHTGBM_C_EXPORT int LGBM_BoosterResetTrainingData(BoosterHandle handle, const DatasetHandle train_data);
LIGHTGBM_C_EXPORT int LGBM_BoosterResetParameter(BoosterHandle handle, const char* parameters);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetNumClasses(BoosterHandle handle, int* out_len);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetLinear(BoosterHandle handle, int* out);
LIGHTGBM_C_EXPORT int LGBM_BoosterUpdateOneIter(BoosterHandle handle, int* is_finished);
LIGHTGBM_C_EXPORT int LGBM_BoosterRefit(BoosterHandle handle, const int32_t* leaf_preds, int32_t nrow, int32_t ncol);
LIGHTGBM_C_EXPORT int LGBM_BoosterUpdateOneIterCustom(BoosterHandle handle, const float* grad, const float* hess,
                                                      int* is_finished);
// One iteration from a custom objective's gradients and hessians in the memory of the GPU the
// booster trains on (anything else is refused). grad_type / hess_type: C_API_DTYPE_FLOAT32 or
// C_API_DTYPE_FLOAT64; value (row i, class k) of an array is ptr[i * row_stride + k *
// class_stride], strides in elements. The arrays have been read when the call returns. Fatal
// for a booster whose score does not live on the device (use LGBM_BoosterUpdateOneIterCustom)
// and for values that are not finite as float32.
LIGHTGBM_C_EXPORT int LGBM_BoosterUpdateOneIterCustomDevice(BoosterHandle handle, const void* grad, const void* hess,
                                                            int grad_type, int hess_type, int32_t nrow,
                                                            int32_t num_class, int64_t grad_row_stride,
                                                            int64_t grad_class_stride, int64_t hess_row_stride,
                                                            int64_t hess_class_stride, int* is_finished);
// The raw (untransformed) class-major fp64 score of the training set (data_idx 0) or validation
// set data_idx - 1, written into caller-owned memory of the training GPU; complete on return.
// out_device_ptr == NULL: only *out_len (values) and *out_device (the GPU's index) are set;
// otherwise *out_len holds the output's capacity on entry and must equal the score's length.
LIGHTGBM_C_EXPORT int LGBM_BoosterGetPredictDevice(BoosterHandle handle, int data_idx, int64_t* out_len,
                                                   int* out_device, double* out_device_ptr);
LIGHTGBM_C_EXPORT int LGBM_BoosterRollbackOneIter(BoosterHandle handle);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetCurrentIteration(BoosterHandle handle, int* out_iteration);
LIGHTGBM_C_EXPORT int LGBM_BoosterNumModelPerIteration(BoosterHandle handle, int* out_tree_per_iteration);
LIGHTGBM_C_EXPORT int LGBM_BoosterNumberOfTotalModel(BoosterHandle handle, int* out_models);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetEvalCounts(BoosterHandle handle, int* out_len);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetEvalNames(BoosterHandle handle, const int len, int* out_len,
                                               const size_t buffer_len, size_t* out_buffer_len, char** out_strs);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetFeatureNames(BoosterHandle handle, const int len, int* out_len,
                                                  const size_t buffer_len, size_t* out_buffer_len, char** out_strs);
LIGHTGBM_C_EXPORT int LGBM_BoosterValidateFeatureNames(BoosterHandle handle, const char** data_names,
                                                       int data_num_features);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetNumFeature(BoosterHandle handle, int* out_len);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetEval(BoosterHandle handle, int data_idx, int* out_len, double* out_results);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetNumPredict(BoosterHandle handle, int data_idx, int64_t* out_len);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetPredict(BoosterHandle handle, int data_idx, int64_t* out_len, double* out_result);
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictForFile(BoosterHandle handle, const char* data_filename,
                                                 int data_has_header, int predict_type, int start_iteration,
                                                 int num_iteration, const char* parameter,
                                                 const char* result_filename);
LIGHTGBM_C_EXPORT int LGBM_BoosterCalcNumPredict(BoosterHandle handle, int num_row, int predict_type,
                                                 int start_iteration, int num_iteration, int64_t* out_len);
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictForCSR(BoosterHandle handle, const void* indptr, int indptr_type,
                                                const int32_t* indices, const void* data, int data_type,
                                                int64_t nindptr, int64_t nelem, int64_t num_col, int predict_type,
                                                int start_iteration, int num_iteration, const char* parameter,
                                                int64_t* out_len, double* out_result);
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictForCSRSingleRow(BoosterHandle handle, const void* indptr, int indptr_type,
                                                         const int32_t* indices, const void* data, int data_type,
                                                         int64_t nindptr, int64_t nelem, int64_t num_col,
                                                         int predict_type, int start_iteration, int num_iteration,
                                                         const char* parameter, int64_t* out_len, double* out_result);
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictForCSC(BoosterHandle handle, const void* col_ptr, int col_ptr_type,
                                                const int32_t* indices, const void* data, int data_type,
                                                int64_t ncol_ptr, int64_t nelem, int64_t num_row, int predict_type,
                                                int start_iteration, int num_iteration, const char* parameter,
                                                int64_t* out_len, double* out_result);
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictForMat(BoosterHandle handle, const void* data, int data_type, int32_t nrow,
                                                int32_t ncol, int is_row_major, int predict_type, int start_iteration,
                                                int num_iteration, const char* parameter, int64_t* out_len,
                                                double* out_result);
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictForMatSingleRow(BoosterHandle handle, const void* data, int data_type,
                                                         int ncol, int is_row_major, int predict_type,
                                                         int start_iteration, int num_iteration,
                                                         const char* parameter, int64_t* out_len, double* out_result);
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictForMats(BoosterHandle handle, const void** data, int data_type, int32_t nrow,
                                                 int32_t ncol, int predict_type, int start_iteration,
                                                 int num_iteration, const char* parameter, int64_t* out_len,
                                                 double* out_result);
// Prediction on the device from a dense row-major matrix (Booster.predict_device). `data` and
// `out_result` may each be host or device memory (data_on_device / out_on_device). RAW_SCORE and
// LEAF_INDEX equal LGBM_BoosterPredictForMat bit for bit; NORMAL with host output too (the host's
// ConvertOutput), NORMAL with device output applies the transform on the device. PREDICT_CONTRIB,
// pred_early_stop=true and a process without a GPU return -1; nothing falls back to the host.
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictForMatDevice(BoosterHandle handle, const void* data, int data_type,
                                                      int32_t nrow, int32_t ncol, int predict_type,
                                                      int start_iteration, int num_iteration, const char* parameter,
                                                      int data_on_device, int out_on_device, int64_t* out_len,
                                                      double* out_result);
// Test hook: the packed ensemble and row walk of the device path, run in a host loop (no GPU).
LIGHTGBM_C_EXPORT int LGBM_BoosterTestPackedPredict(BoosterHandle handle, const void* data, int data_type,
                                                    int32_t nrow, int32_t ncol, int predict_type, int start_iteration,
                                                    int num_iteration, const char* parameter, int64_t* out_len,
                                                    double* out_result);
// Test hook: the same result by the tree-parallel algorithm of the resident predictor's small-batch
// kernels, in host loops (no GPU): every (row, tree) pair into a [tree][row] array, then the fold.
LIGHTGBM_C_EXPORT int LGBM_BoosterTestPackedPredictTreeParallel(BoosterHandle handle, const void* data,
                                                                int data_type, int32_t nrow, int32_t ncol,
                                                                int predict_type, int start_iteration,
                                                                int num_iteration, const char* parameter,
                                                                int64_t* out_len, double* out_result);
// A resident device predictor (Booster.device_predictor): the iterations LGBM_BoosterPredictForMatDevice
// would select are packed and uploaded once and `parameter` is parsed once; every later call only
// moves rows and launches. The predictor is a snapshot: later changes of the booster's trees do
// not reach it. The booster must outlive it (its objective transforms NORMAL output).
// tree_parallel_rows: batches of at most this many rows run the tree-parallel kernels (one work
// item per row and tree), larger ones the row-parallel kernels; 0 never, -1 the measured default,
// more than 65536 is an error. pred_early_stop=true and a process without a GPU return -1.
LIGHTGBM_C_EXPORT int LGBM_BoosterDevicePredictorCreate(BoosterHandle handle, int start_iteration, int num_iteration,
                                                        int tree_parallel_rows, const char* parameter,
                                                        DevicePredictorHandle* out);
// Arguments and results as LGBM_BoosterPredictForMatDevice's, PREDICT_CONTRIB refused. Calls on
// one handle are serialised inside it.
LIGHTGBM_C_EXPORT int LGBM_DevicePredictorPredict(DevicePredictorHandle handle, const void* data, int data_type,
                                                  int32_t nrow, int32_t ncol, int predict_type, int data_on_device,
                                                  int out_on_device, int64_t* out_len, double* out_result);
// The kernel family of the last call that launched: 0 row-parallel, 1 tree-parallel, -1 none yet.
LIGHTGBM_C_EXPORT int LGBM_DevicePredictorLastPath(DevicePredictorHandle handle, int* out);
LIGHTGBM_C_EXPORT int LGBM_DevicePredictorFree(DevicePredictorHandle handle);
// SHAP values on the device from a dense row-major matrix (Booster.predict_contrib_device):
// nrow x trees-per-iteration x (features + 1) doubles, the layout and length of PREDICT_CONTRIB
// (LGBM_BoosterCalcNumPredict). `data` and `out_result` may each be host memory or memory of the
// current device. The values equal LGBM_BoosterPredictForMat's to rounding (the sums are
// associated in another order); the last column of each class block, the expected value, bit for
// bit. Returns -1, with nothing falling back to the host, for a process without a GPU,
// pred_early_stop=true, a model with linear trees, and a root-to-leaf path that splits on more
// than 64 distinct features (kCMaxPathFeatures, src/device/contrib_pack.h).
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictContribForMatDevice(BoosterHandle handle, const void* data, int data_type,
                                                             int32_t nrow, int32_t ncol, int start_iteration,
                                                             int num_iteration, const char* parameter,
                                                             int data_on_device, int out_on_device, int64_t* out_len,
                                                             double* out_result);
// Test hook: the path pack and per-row function of the device path, run in a host loop (no GPU).
LIGHTGBM_C_EXPORT int LGBM_BoosterTestPackedContrib(BoosterHandle handle, const void* data, int data_type,
                                                    int32_t nrow, int32_t ncol, int start_iteration,
                                                    int num_iteration, const char* parameter, int64_t* out_len,
                                                    double* out_result);
// A Dataset from dense matrices that already live on the GPU (torch tensors): nmat row chunks of
// ncol columns, fp32 or fp64, chunk i holding value (r, c) at data[i][r * row_stride[i] +
// c * col_stride[i]] (strides in elements, so views are read in place). The bin-construction
// sample is gathered on the device, the rows are binned there whatever device_type and
// device_binning say; mappers, bundles and bins equal LGBM_DatasetCreateFromMat(s) on the same
// values. The caller's work on the chunks must be complete. A process without a GPU returns -1.
LIGHTGBM_C_EXPORT int LGBM_DatasetCreateFromDeviceMats(int32_t nmat, const void** data, int data_type,
                                                       const int32_t* nrow, int32_t ncol, const int64_t* row_stride,
                                                       const int64_t* col_stride, const char* parameters,
                                                       const DatasetHandle reference, DatasetHandle* out);
// Test hook: the same construction over host matrices, gather and packing in host loops (no GPU).
LIGHTGBM_C_EXPORT int LGBM_DatasetTestCreateFromSampledMats(int32_t nmat, const void** data, int data_type,
                                                            const int32_t* nrow, int32_t ncol,
                                                            const int64_t* row_stride, const int64_t* col_stride,
                                                            const char* parameters, const DatasetHandle reference,
                                                            DatasetHandle* out);
LIGHTGBM_C_EXPORT int LGBM_BoosterSaveModel(BoosterHandle handle, int start_iteration, int num_iteration,
                                            int feature_importance_type, const char* filename);
LIGHTGBM_C_EXPORT int LGBM_BoosterSaveModelToString(BoosterHandle handle, int start_iteration, int num_iteration,
                                                    int feature_importance_type, int64_t buffer_len, int64_t* out_len,
                                                    char* out_str);
LIGHTGBM_C_EXPORT int LGBM_BoosterDumpModel(BoosterHandle handle, int start_iteration, int num_iteration,
                                            int feature_importance_type, int64_t buffer_len, int64_t* out_len,
                                            char* out_str);
LIGHTGBM_C_EXPORT int LGBM_BoosterConvertModelToIfElse(BoosterHandle handle, int num_iteration, int64_t buffer_len,
                                                       int64_t* out_len, char* out_str);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetLeafValue(BoosterHandle handle, int tree_idx, int leaf_idx, double* out_val);
LIGHTGBM_C_EXPORT int LGBM_BoosterSetLeafValue(BoosterHandle handle, int tree_idx, int leaf_idx, double val);
LIGHTGBM_C_EXPORT int LGBM_BoosterFeatureImportance(BoosterHandle handle, int num_iteration, int importance_type,
                                                    double* out_results);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetUpperBoundValue(BoosterHandle handle, double* out_results);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetLowerBoundValue(BoosterHandle handle, double* out_results);
LIGHTGBM_C_EXPORT int LGBM_BoosterGetDeviceName(BoosterHandle handle, int64_t buffer_len, int64_t* out_len,
                                                char* out_str);

/* ---- Network */
LIGHTGBM_C_EXPORT int LGBM_NetworkInit(const char* machines, int local_listen_port, int listen_time_out,
                                       int num_machines);
LIGHTGBM_C_EXPORT int LGBM_NetworkFree();
LIGHTGBM_C_EXPORT int LGBM_NetworkInitWithFunctions(int num_machines, int rank, void* reduce_scatter_ext_fun,
                                                    void* allgather_ext_fun);
LIGHTGBM_C_EXPORT int LGBM_SetMaxThreads(int num_threads);
LIGHTGBM_C_EXPORT int LGBM_GetMaxThreads(int* out);
LIGHTGBM_C_EXPORT int LGBM_GetEffectiveThreads(int* out);

/* ---- Arrow C data interface (struct ArrowArray / ArrowSchema, see lgap/arrow.h) */
struct ArrowArray;
struct ArrowSchema;
typedef void* ByteBufferHandle;
#define C_API_MATRIX_TYPE_CSR (0)
#define C_API_MATRIX_TYPE_CSC (1)
LIGHTGBM_C_EXPORT int LGBM_DatasetCreateFromArrow(int64_t n_chunks, const struct ArrowArray* chunks,
                                                  const struct ArrowSchema* schema, const char* parameters,
                                                  const DatasetHandle reference, DatasetHandle* out);
LIGHTGBM_C_EXPORT int LGBM_DatasetSetFieldFromArrow(DatasetHandle handle, const char* field_name, int64_t n_chunks,
                                                    const struct ArrowArray* chunks, const struct ArrowSchema* schema);
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictForArrow(BoosterHandle handle, int64_t n_chunks,
                                                  const struct ArrowArray* chunks, const struct ArrowSchema* schema,
                                                  int predict_type, int start_iteration, int num_iteration,
                                                  const char* parameter, int64_t* out_len, double* out_result);

/* ---- more dataset constructors */
// get_row_funptr: std::function<void(int idx, std::vector<std::pair<int, double>>& row)>*
LIGHTGBM_C_EXPORT int LGBM_DatasetCreateFromCSRFunc(void* get_row_funptr, int num_rows, int64_t num_col,
                                                    const char* parameters, const DatasetHandle reference,
                                                    DatasetHandle* out);
LIGHTGBM_C_EXPORT int LGBM_DatasetCreateFromSampledColumn(double** sample_data, int** sample_indices, int32_t ncol,
                                                          const int* num_per_col, int32_t num_sample_row,
                                                          int32_t num_local_row, int64_t num_dist_row,
                                                          const char* parameters, DatasetHandle* out);
LIGHTGBM_C_EXPORT int LGBM_DatasetPushRowsByCSRWithMetadata(DatasetHandle dataset, const void* indptr,
                                                            int indptr_type, const int32_t* indices, const void* data,
                                                            int data_type, int64_t nindptr, int64_t nelem,
                                                            int64_t start_row, const float* label, const float* weight,
                                                            const double* init_score, const int32_t* query,
                                                            int32_t tid);
LIGHTGBM_C_EXPORT int LGBM_DatasetSerializeReferenceToBinary(DatasetHandle handle, ByteBufferHandle* out,
                                                             int32_t* out_len);
LIGHTGBM_C_EXPORT int LGBM_DatasetCreateFromSerializedReference(const void* ref_buffer, int32_t ref_buffer_size,
                                                                int64_t num_row, int32_t num_classes,
                                                                const char* parameters, DatasetHandle* out);
LIGHTGBM_C_EXPORT int LGBM_ByteBufferGetAt(ByteBufferHandle handle, int32_t index, uint8_t* out_val);
LIGHTGBM_C_EXPORT int LGBM_ByteBufferFree(ByteBufferHandle handle);

/* ---- single-row fast prediction (config parsed once) */
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictForMatSingleRowFastInit(BoosterHandle handle, const int predict_type,
                                                                 const int start_iteration, const int num_iteration,
                                                                 const int data_type, const int32_t ncol,
                                                                 const char* parameter,
                                                                 FastConfigHandle* out_fastConfig);
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictForMatSingleRowFast(FastConfigHandle fastConfig_handle, const void* data,
                                                             int64_t* out_len, double* out_result);
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictForCSRSingleRowFastInit(BoosterHandle handle, const int predict_type,
                                                                 const int start_iteration, const int num_iteration,
                                                                 const int data_type, const int64_t num_col,
                                                                 const char* parameter,
                                                                 FastConfigHandle* out_fastConfig);
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictForCSRSingleRowFast(FastConfigHandle fastConfig_handle, const void* indptr,
                                                             const int indptr_type, const int32_t* indices,
                                                             const void* data, const int64_t nindptr,
                                                             const int64_t nelem, int64_t* out_len,
                                                             double* out_result);
LIGHTGBM_C_EXPORT int LGBM_FastConfigFree(FastConfigHandle fastConfig);

/* ---- sparse SHAP output */
LIGHTGBM_C_EXPORT int LGBM_BoosterPredictSparseOutput(BoosterHandle handle, const void* indptr, int indptr_type,
                                                      const int32_t* indices, const void* data, int data_type,
                                                      int64_t nindptr, int64_t nelem, int64_t num_col_or_row,
                                                      int predict_type, int start_iteration, int num_iteration,
                                                      const char* parameter, int matrix_type, int64_t* out_len,
                                                      void** out_indptr, int32_t** out_indices, void** out_data);
LIGHTGBM_C_EXPORT int LGBM_BoosterFreePredictSparse(void* indptr, int32_t* indices, void* data, int indptr_type,
                                                    int data_type);
LIGHTGBM_C_EXPORT void LGBM_SetLastError(const char* msg);

/* ---- MI355X device helpers (LambdaGap extension) */
LIGHTGBM_C_EXPORT int LGBM_DeviceCount(int* out);
// Waits for all queued device work of this process (timing brackets).
LIGHTGBM_C_EXPORT int LGBM_DeviceSynchronize();
// ---- kernel-level entry points (numerics tests / ops module)
// Gradients and hessians of the last boosting round (class-major); pass null buffers to query *out_len.
LIGHTGBM_C_EXPORT int LGBM_BoosterGetGradients(BoosterHandle handle, int64_t* out_len, float* grad, float* hess);
// Learned position biases of a lambdarank booster trained with positions, by position id (read-only; 0 without
// positions); pass a null buffer to query *out_len.
LIGHTGBM_C_EXPORT int LGBM_BoosterGetPositionBiases(BoosterHandle handle, int64_t* out_len, double* out);
// Packed group layout: groups, total histogram bins, bytes per group bin, per-group histogram start.
LIGHTGBM_C_EXPORT int LGBM_DatasetGetGroupLayout(DatasetHandle handle, int* num_groups, int* num_total_bin,
                                                 int* bin_width, int32_t* hist_start);
// Row-major [num_data x num_groups] group bins.
LIGHTGBM_C_EXPORT int LGBM_DatasetGetGroupBins(DatasetHandle handle, uint16_t* out);
// (grad, hess) histogram over `rows` (null = all rows) built by the HIP histogram kernel:
// out_hist has 2 * num_total_bin doubles; group bin 0 (all features at their most frequent bin) stays 0.
LIGHTGBM_C_EXPORT int LGBM_DeviceHistogram(DatasetHandle handle, const float* grad, const float* hess,
                                           const int32_t* rows, int32_t num_rows, double* out_hist);
// Direct tests of the frontier engine's production kernels with a device learner configured by
// `parameters`: k_f_hist over k row subsets (rows concatenated, offsets[k + 1]) -> out
// [k][num_total_bin][2] at the kernel's fixed-point scale (quantized: integer level sums, levels
// [num_data] = g level << 8 | h level); k_f_partition of k parents -> the device's children lists
// and left counts next to the host learner's stable partition (exp_*).
LIGHTGBM_C_EXPORT int LGBM_DeviceTestFrontierHist(DatasetHandle handle, const char* parameters, const float* grad,
                                                  const float* hess, const int32_t* rows, const int32_t* offsets,
                                                  int k, double* out, uint16_t* levels);
// k_f_scan of the root round (all rows) next to the host split_math.h scan of the same histogram:
// out / ref [num_features][8] (gain, threshold, left count, default_left, left sum g, left sum h,
// valid, categorical thresholds).
LIGHTGBM_C_EXPORT int LGBM_DeviceTestFrontierScan(DatasetHandle handle, const char* parameters, const float* grad,
                                                  const float* hess, double* out, double* ref);
LIGHTGBM_C_EXPORT int LGBM_DeviceTestFrontierPartition(DatasetHandle handle, const char* parameters,
                                                       const int32_t* rows, const int32_t* offsets, int k,
                                                       const int32_t* feats, const int32_t* thr, const int32_t* dleft,
                                                       const uint32_t* catbits, int32_t* out_rows, int32_t* out_left,
                                                       int32_t* exp_rows, int32_t* exp_left);
// The gradient quantizer of a device learner configured by `parameters` (use_quantized_grad),
// run as training runs it: grad / hess [num_class][num_data] uploaded every round, then quantized
// class by class, `rounds` times. Outputs per (round, class): out_gh [num_data][2] de-quantized
// (g, h); out_levels [num_data] g level << 8 | h level, valid when *out_has_levels != 0;
// out_qmax [2] float bits of max |g|, max |h|; out_true [num_data][2] the inputs kept for
// quant_train_renew_leaf (untouched otherwise).
LIGHTGBM_C_EXPORT int LGBM_DeviceTestQuantize(DatasetHandle handle, const char* parameters, int const_hess,
                                              const float* grad, const float* hess, int num_class, int rounds,
                                              float* out_gh, uint16_t* out_levels, uint32_t* out_qmax,
                                              float* out_true, int* out_has_levels);
// One launch of the linear-leaf Gram kernels over host arrays: raw [num_data][num_feature], leaf
// l's rows by segs[3 l ..] = (0, start, count) into `rows` or (-1, start, count) for the
// contiguous rows start .. start + count, its features feats[feat_off[l] .. feat_off[l + 1])
// (sorted). out [num_leaves][64][64] holds A in rows / columns [0, m) and c in column m
// (m = features + 1), out_usable [num_leaves] the non-NaN values read before each row's first NaN.
LIGHTGBM_C_EXPORT int LGBM_DeviceTestLinearGram(const float* raw, int32_t num_data, int32_t num_feature,
                                                const float* grad, const float* hess, const int32_t* rows,
                                                int32_t num_rows, const int32_t* segs, int num_leaves,
                                                const int32_t* feat_off, const int32_t* feats, int chunks,
                                                double* out, int64_t* out_usable);
// The forest traversal (k_traverse_forest) with a device learner on the Dataset: trees
// tree_idx[0 .. num_trees) of the booster, tree j's leaf values times scales[j] (Tree::Shrinkage on
// a copy), are added in list order into a copy of score [num_data], returned in out. grid > 0 caps
// the kernel's grid; per_tree != 0 runs one single-tree traversal per tree instead. out_info (may
// be null) [2]: the group-bin width of the rows read (0 = 4-bit rows, 1, 2 bytes), dwords per row.
LIGHTGBM_C_EXPORT int LGBM_DeviceTestForestScore(DatasetHandle handle, BoosterHandle booster, const int32_t* tree_idx,
                                                 const double* scales, int num_trees, const double* score, int grid,
                                                 int per_tree, double* out, int32_t* out_info);
// Direct test of the blended score update (boosting=rf's running average) over the packed rows of a
// constructed Dataset: tree tree_idx of booster is blended into a copy of score [num_data], out[i] =
// divide ? (score[i] * pre + tree(i)) / post : (score[i] * pre + tree(i)) * post, three fp64
// roundings. grid > 0 caps the kernel's grid.
LIGHTGBM_C_EXPORT int LGBM_DeviceTestBlendScore(DatasetHandle handle, BoosterHandle booster, int tree_idx,
                                                const double* score, double pre, double post, int divide, int grid,
                                                double* out);
// How that forest is split into LDS runs (no GPU needed): out_run_trees [num_trees] the trees per
// run, out_run_bytes [num_trees] their bytes, *out_num_runs, and *out_budget the run byte budget.
LIGHTGBM_C_EXPORT int LGBM_DeviceTestForestRuns(BoosterHandle booster, const int32_t* tree_idx, int num_trees,
                                                int32_t* out_run_trees, int32_t* out_run_bytes, int* out_num_runs,
                                                int* out_budget);
// One device row-sampling pass (the HIP bagging / GOSS kernels) over host arrays: mode 1 bagging,
// 2 balanced bagging, 3 GOSS; `rounds` > 1 re-bags with the advanced streams and reports the last.
// grad/hess (num_class * num_rows, class-major) are scaled in place by GOSS. Returns the kept
// rows (ascending) in out_rows and their count in out_count.
LIGHTGBM_C_EXPORT int LGBM_DeviceSampleRows(int mode, int32_t num_rows, int num_class, float* grad, float* hess,
                                            const float* label, double fraction, double pos_fraction,
                                            double neg_fraction, double top_rate, double other_rate,
                                            int bagging_seed, uint32_t goss_seed, int rounds, int32_t* out_rows,
                                            int32_t* out_count);
// The same kernels for a direct test: also mode 4, bagging by query (query_sizes[num_queries] sum to
// num_rows; the per-query streams are advanced after every round as the learner does), and with_oob
// != 0 the out-of-bag list. out_rows and out_oob (may be null without with_oob), both [num_rows], are
// filled with -1 before every round and returned whole: the kept rows in out_rows[0 .. *out_total),
// the others in out_oob[0 .. num_rows - *out_total), -1 wherever the kernels did not write.
LIGHTGBM_C_EXPORT int LGBM_DeviceTestSampleRows(int mode, int32_t num_rows, int num_class, float* grad, float* hess,
                                                const float* label, const int32_t* query_sizes, int32_t num_queries,
                                                double fraction, double pos_fraction, double neg_fraction,
                                                double top_rate, double other_rate, int bagging_seed,
                                                uint32_t goss_seed, int rounds, int with_oob, int32_t* out_rows,
                                                int32_t* out_oob, int32_t* out_total);
// The host sampler those kernels reproduce (no GPU needed): a SampleStrategy with `parameters` over the
// Dataset, Bagging(iters[i], grad, hess) for every i in order. grad/hess (num_class * num_data,
// class-major) are scaled in place by GOSS. out_indices [num_data]: bag_indices(), the bag followed by
// the out-of-bag rows; *out_bag_cnt: bag_cnt(); *out_drawn: whether the last call drew a bag (if none
// ever did, every row is used and out_indices holds no list).
LIGHTGBM_C_EXPORT int LGBM_TestHostSampleRows(DatasetHandle handle, const char* parameters, int num_class,
                                              const int32_t* iters, int num_iters, float* grad, float* hess,
                                              int32_t* out_indices, int32_t* out_bag_cnt, int* out_drawn);
LIGHTGBM_C_EXPORT int LGBM_DeviceCommGetUniqueId(char* out, int64_t buffer_len, int64_t* out_len);
LIGHTGBM_C_EXPORT int LGBM_DeviceCommInit(const char* unique_id, int64_t id_len, int num_ranks, int rank,
                                          int device_id);
LIGHTGBM_C_EXPORT int LGBM_DeviceCommFree();
LIGHTGBM_C_EXPORT int LGBM_PhaseTimerReport(int64_t buffer_len, int64_t* out_len, char* out_str);

#endif /* LGAP_C_API_H_ */
