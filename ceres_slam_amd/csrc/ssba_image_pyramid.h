// The image pyramid of the dense driver (ssba_image_pyramid_create, ssba_image_pyramid.hip): every level of the pair in device
// memory.  ssba_api.hip reads a level's four images when ssba_add_image_level binds it to a handle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

struct ssba_image_pyramid {
    struct Level {
        int rows = 0, cols = 0;
        uint8_t *u8[2] = {nullptr, nullptr};                       // reference, tracked: the rounded 8-bit level
        double *img[4] = {nullptr, nullptr, nullptr, nullptr};     // ref, track, gradx, grady
        double *disp = nullptr;                                    // levels >= disparity_level
    };
    int device = 0;
    int disparity_level = 0, gradient_source = 0;
    double gradient_scale = 1.0;
    double huber_a = 0.0;                                          // ssba_image_pyramid_set_huber_loss: every level's handle gets it
    hipStream_t stream = nullptr;
    std::vector<Level> lv;
    std::vector<void *> allocs;
};
