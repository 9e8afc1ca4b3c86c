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
    bool borrowed = false;                                         // ssba_image_sequence_pyramid: levels, stream and memory are the sequence's
};

// A stereo sequence of F frames (ssba_image_sequence_create): per level one frame-major buffer each for the 8-bit images (the F
// left frames, then the F - 1 right frames down to disparity_level), the double images, both gradients, and from disparity_level
// on the F - 1 disparity maps.  pairs[k] is the borrowed pyramid of pair k: its level pointers lie in these buffers.
struct ssba_image_sequence {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<void *> allocs;
    std::vector<ssba_image_pyramid *> pairs;
};
