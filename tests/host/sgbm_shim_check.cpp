// What ceres_slam::StereoSGBM and the ImagePyramid constructor that takes the right image refuse: every case is refused by the C
// call before it looks for a device (ssba_stereo_sgbm / ssba_image_pyramid_create_stereo judge their arguments first), so the
// shim throws std::invalid_argument without a GPU.  tests/test_host_sgbm.py builds and runs this program.
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
    const int rows = 64, cols = 96;
    std::vector<uint8_t> a((size_t)rows * cols, 10), b(a), c(a);
    const ceres_slam::Image8 left(rows, cols, a.data()), right(rows, cols, b.data()), narrow(rows, cols - 1, b.data());
    ceres_slam::DisparityMap disp;

    {   // the driver's call shape and its defaults
        ceres_slam::StereoSGBM sgbm(0, 64, 15);
        const ssba_sgbm_params &q = sgbm.params;
        if (q.min_disparity != 0 || q.num_disparities != 64 || q.block_size != 15 || q.p1 || q.p2 || q.disp12_max_diff || q.pre_filter_cap ||
            q.uniqueness_ratio || q.speckle_window_size || q.speckle_range || q.full_dp) {
            std::printf("FAIL defaults\n");
            ++failures;
        }
    }
    const char *call = "ssba_stereo_sgbm";
    refused("negative minimum disparity", call, [&] { ceres_slam::StereoSGBM(-1, 64, 15)(left, right, disp); });
    refused("24 disparities", call, [&] { ceres_slam::StereoSGBM(0, 24, 15)(left, right, disp); });
    refused("272 disparities", call, [&] { ceres_slam::StereoSGBM(0, 272, 15)(left, right, disp); });
    refused("even block", call, [&] { ceres_slam::StereoSGBM(0, 64, 4)(left, right, disp); });
    refused("block 17", call, [&] { ceres_slam::StereoSGBM(0, 64, 17)(left, right, disp); });
    refused("uniqueness 101", call, [&] { ceres_slam::StereoSGBM(0, 64, 15, 0, 0, 0, 0, 101)(left, right, disp); });
    refused("pre-filter cap 128", call, [&] { ceres_slam::StereoSGBM(0, 64, 15, 0, 0, 0, 128)(left, right, disp); });
    refused("P2 past 16 bits", call, [&] { ceres_slam::StereoSGBM(0, 64, 15, 8, 65535 - 20925 + 1)(left, right, disp); });
    refused("speckle window", "speckle", [&] { ceres_slam::StereoSGBM(0, 64, 15, 0, 0, 0, 0, 0, 50)(left, right, disp); });
    refused("speckle range", "speckle", [&] { ceres_slam::StereoSGBM(0, 64, 15, 0, 0, 0, 0, 0, 0, 2)(left, right, disp); });
    refused("full DP", call, [&] { ceres_slam::StereoSGBM(0, 64, 15, 0, 0, 0, 0, 0, 0, 0, true)(left, right, disp); });
    refused("no computable column", call, [&] { ceres_slam::StereoSGBM(40, 64, 15)(left, right, disp); });
    refused("two sizes", "one size", [&] { ceres_slam::StereoSGBM(0, 64, 15)(left, narrow, disp); });

    call = "ssba_image_pyramid_create_stereo";
    const ceres_slam::StereoSGBM ok(0, 16, 5);
    refused("pyramid: 24 disparities", call, [&] { ceres_slam::ImagePyramid(a.data(), b.data(), c.data(), rows, cols, 3, 0, ceres_slam::StereoSGBM(0, 24, 5)); });
    refused("pyramid: speckle window", "speckle",
            [&] { ceres_slam::ImagePyramid(a.data(), b.data(), c.data(), rows, cols, 3, 0, ceres_slam::StereoSGBM(0, 16, 5, 0, 0, 0, 0, 0, 50)); });
    refused("pyramid: no computable column at the matcher's level", call, [&] { ceres_slam::ImagePyramid(a.data(), b.data(), c.data(), rows, cols, 3, 2, ceres_slam::StereoSGBM(0, 32, 5)); });   // 16 x 24
    refused("pyramid: NULL right image", call, [&] { ceres_slam::ImagePyramid(a.data(), (const uint8_t *)NULL, c.data(), rows, cols, 3, 0, ok); });
    refused("pyramid: disparity_level = levels", call, [&] { ceres_slam::ImagePyramid(a.data(), b.data(), c.data(), rows, cols, 3, 3, ok); });
    refused("pyramid: a level below 8 rows", call, [&] { ceres_slam::ImagePyramid(a.data(), b.data(), c.data(), rows, cols, 5, 0, ok); });
    refused("pyramid: zero gradient scale", call, [&] { ceres_slam::ImagePyramid(a.data(), b.data(), c.data(), rows, cols, 3, 0, ok, SSBA_GRADIENT_OF_TRACKED, 0.0); });

    if (failures) {
        std::printf("%d FAILures\n", failures);
        return 1;
    }
    std::printf("all refusals hold\n");
    return 0;
}
