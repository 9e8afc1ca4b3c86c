// What ceres_slam::ImageSequence and the batched call of ceres_slam::StereoSGBM refuse: every case is refused by the C call before
// it looks for a device (ssba_image_sequence_create / ssba_stereo_sgbm_batch judge their arguments first) or by the shim itself, so
// std::invalid_argument is thrown without a GPU.  tests/test_host_image_sequence.py builds and runs this program.
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "ceres_slam_amd/ceres_shim.hpp"

static int failures = 0;

template <class F> static void refused(const char *what, const char *needle, F f) {
    try {
        f();
        std::printf("FAIL %s: no exception\n", what);
        ++failures;
    } catch (const std::invalid_argument &e) {
        if (std::string(e.what()).find(needle) == std::string::npos) {
            std::printf("FAIL %s: message '%s' lacks '%s'\n", what, e.what(), needle);
            ++failures;
        } else {
            std::printf("ok   %s: %s\n", what, e.what());
        }
    } catch (const std::exception &e) {
        std::printf("FAIL %s: another exception: %s\n", what, e.what());
        ++failures;
    }
}

int main() {
    const int rows = 64, cols = 96, frames = 3;
    const size_t npix = (size_t)rows * cols;
    std::vector<uint8_t> left(npix * frames, 10), right(npix * frames, 12);
    const ceres_slam::StereoSGBM ok(0, 16, 5);
    using ceres_slam::ImageSequence;
    using ceres_slam::StereoSGBM;

    const char *call = "ssba_image_sequence_create";
    refused("one frame", call, [&] { ImageSequence(left.data(), right.data(), 1, rows, cols, 3, 0, ok); });
    refused("NULL left stack", call, [&] { ImageSequence((const uint8_t *)NULL, right.data(), frames, rows, cols, 3, 0, ok); });
    refused("NULL right stack", call, [&] { ImageSequence(left.data(), (const uint8_t *)NULL, frames, rows, cols, 3, 0, ok); });
    refused("levels = 0", call, [&] { ImageSequence(left.data(), right.data(), frames, rows, cols, 0, 0, ok); });
    refused("disparity_level = levels", call, [&] { ImageSequence(left.data(), right.data(), frames, rows, cols, 3, 3, ok); });
    refused("a level below 8 rows", call, [&] { ImageSequence(left.data(), right.data(), frames, rows, cols, 5, 0, ok); });
    refused("unknown gradient source", call, [&] { ImageSequence(left.data(), right.data(), frames, rows, cols, 3, 0, ok, 2); });
    refused("zero gradient scale", call, [&] { ImageSequence(left.data(), right.data(), frames, rows, cols, 3, 0, ok, SSBA_GRADIENT_OF_TRACKED, 0.0); });
    refused("24 disparities", call, [&] { ImageSequence(left.data(), right.data(), frames, rows, cols, 3, 0, StereoSGBM(0, 24, 5)); });
    refused("speckle window", "speckle", [&] { ImageSequence(left.data(), right.data(), frames, rows, cols, 3, 0, StereoSGBM(0, 16, 5, 0, 0, 0, 0, 0, 50)); });
    refused("no computable column at the matcher's level", call, [&] { ImageSequence(left.data(), right.data(), frames, rows, cols, 3, 2, StereoSGBM(0, 32, 5)); });
    // one pair at 64 x 96, D 16: 12 * 64 * 80 * 16 = 983040 bytes
    refused("workspace below one pair", "983040", [&] { ImageSequence(left.data(), right.data(), frames, rows, cols, 3, 0, ok, SSBA_GRADIENT_OF_TRACKED, 0.125, 983039); });
    {
        std::vector<const uint8_t *> l{left.data(), left.data() + npix, left.data() + 2 * npix}, r1{right.data()}, rn{right.data(), NULL};
        refused("one right frame for three left frames", "right frames", [&] { ImageSequence(l, r1, rows, cols, 3, 0, ok); });
        refused("a NULL frame", "NULL frame", [&] { ImageSequence(l, rn, rows, cols, 3, 0, ok); });
        refused("one left frame", "right frames", [&] { ImageSequence(r1, r1, rows, cols, 3, 0, ok); });
    }

    call = "ssba_stereo_sgbm_batch";
    const ceres_slam::Image8 a(rows, cols, left.data()), b(rows, cols, right.data()), narrow(rows, cols - 1, right.data());
    std::vector<ceres_slam::DisparityMap> maps;
    const std::vector<ceres_slam::Image8> two_l{a, a}, two_r{b, b}, one_r{b}, mixed{b, narrow}, none;
    refused("batch: no pair", call, [&] { ok(none, none, maps); });
    refused("batch: two left, one right", "as many", [&] { ok(two_l, one_r, maps); });
    refused("batch: two sizes", "one size", [&] { ok(two_l, mixed, maps); });
    refused("batch: 24 disparities", call, [&] { StereoSGBM(0, 24, 5)(two_l, two_r, maps); });
    refused("batch: even block", call, [&] { StereoSGBM(0, 16, 4)(two_l, two_r, maps); });
    refused("batch: full DP", call, [&] { StereoSGBM(0, 16, 5, 0, 0, 0, 0, 0, 0, 0, true)(two_l, two_r, maps); });
    refused("batch: speckle range", "speckle", [&] { StereoSGBM(0, 16, 5, 0, 0, 0, 0, 0, 0, 2)(two_l, two_r, maps); });
    refused("batch: no computable column", call, [&] { StereoSGBM(90, 16, 5)(two_l, two_r, maps); });
    refused("batch: workspace below one pair", "983040", [&] { ok(two_l, two_r, maps, 1000); });

    if (failures) {
        std::printf("%d FAILures\n", failures);
        return 1;
    }
    std::printf("all refusals hold\n");
    return 0;
}
