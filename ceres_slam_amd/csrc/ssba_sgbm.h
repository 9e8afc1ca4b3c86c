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

}  // namespace ssba
