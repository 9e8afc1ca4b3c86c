// The semi-global matcher (ssba_sgbm.hip) as the pyramid calls it: the parameter check and the launches on a caller's stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/ssba.h"

namespace ssba {

struct SgbmPlan {
    int rows, cols, W, D, min_d, maxD, r, cap, P1, P2, uniq, lr;
};

// SSBA_OK and the plan, or the refusal with ssba_last_error set ("<call>: ...")
int sgbm_check(const char *call, uint32_t rows, uint32_t cols, const ssba_sgbm_params *params, SgbmPlan *plan);
// Enqueues the matcher on `s`: left / right are device images (rows * cols bytes), disp16 / disparity device outputs (either may
// be nullptr).  The volumes come from the pool and are appended to `temps`: the caller frees them once `s` has been synchronised.
hipError_t sgbm_enqueue(const SgbmPlan &plan, const uint8_t *left, const uint8_t *right, int16_t *disp16, double *disparity, hipStream_t s,
                        std::vector<void *> *temps);

// The batched matcher.  sgbm_pair_bytes: the six 16-bit volumes of one pair.  sgbm_chunk_pairs: how many pairs one chunk holds
// under workspace_bytes (0: SSBA_SGBM_DEFAULT_WORKSPACE_BYTES), at most n; refuses a bound below one pair.
uint64_t sgbm_pair_bytes(const SgbmPlan &plan);
int sgbm_chunk_pairs(const char *call, const SgbmPlan &plan, uint32_t n, uint64_t workspace_bytes, uint32_t *pairs);
// sgbm_enqueue over n pairs in chunks of chunk_pairs, five launches per chunk: pair k's images are left / right + k * img_stride,
// its outputs disp16 / disparity + k * rows * cols.
hipError_t sgbm_enqueue_batch(const SgbmPlan &plan, const uint8_t *left, const uint8_t *right, size_t img_stride, uint32_t n, uint32_t chunk_pairs,
                              int16_t *disp16, double *disparity, hipStream_t s, std::vector<void *> *temps);

}  // namespace ssba
