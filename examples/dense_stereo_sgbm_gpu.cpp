// dense_stereo_sgbm_gpu -- the reference's dense photometric driver from :52 to :136 (tests/dense_stereo_test.cpp) written against
// include/ceres_slam_amd/ceres_shim.hpp.  Of the reference's main only imread is left out: this driver reads the raw 8-bit triple
// left0, right0, left1 from a file -- NO disparity map -- and needs no OpenCV; pyrDown, StereoSGBM, convertTo and Sobel (:52-72) run
// on the device (ceres_slam::ImagePyramid with a ceres_slam::StereoSGBM), and the residual blocks are built on the images of the
// level at which the matcher ran:
//
//     int32  rows, cols, levels, disparity_level, interpolation (0 nearest, 1 bilinear), disparities_constant (0 | 1),
//            gradient_source (0 reference image, as :70-72 stands; 1 tracked image)
//     double gradient_scale, fu, fv, cu, cv, b          the camera of level 0
//     double T_track_ref[12]                            the start, [t | R row-major]
//     int32  min_disparity, num_disparities, block_size, p1, p2, disp12_max_diff, pre_filter_cap, uniqueness_ratio,
//            speckle_window_size, speckle_range, full_dp     the matcher's parameters (ssba_sgbm_params)
//     uint8  left0, right0, left1                       rows * cols each, row-major
//
// usage: dense_stereo_sgbm_gpu triple.raw [--coarse-to-fine <coarsest_level>] [--max-iterations <n>]
// Without --coarse-to-fine: one solve on level disparity_level, the reference's loop (:94-136) with the camera scaled to that
// level.  With it: one solve per level from coarsest_level down to disparity_level, the pose carried along
// (ceres::SolveCoarseToFine); a line "level <l> <BriefReport>" per level.
// Output (17 significant digits): "valid <pixels the matcher accepted>", "blocks n", "report <BriefReport of the last level>", "steps <successful> <unsuccessful>",
// "pose <12>", and with free disparities "disparity_sum <sum over the blocks>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <vector>

#include "ceres_slam_amd/ceres_shim.hpp"

int main(int argc, char **argv) {
    if (argc < 2) {
        std::cerr << "usage: dense_stereo_sgbm_gpu triple.raw [--coarse-to-fine <coarsest_level>] [--max-iterations <n>]" << std::endl;
        return EXIT_FAILURE;
    }
    int coarsest = -1, max_iterations = -1;
    for (int a = 2; a + 1 < argc; a += 2) {
        if (!std::strcmp(argv[a], "--coarse-to-fine")) coarsest = std::atoi(argv[a + 1]);
        else if (!std::strcmp(argv[a], "--max-iterations")) max_iterations = std::atoi(argv[a + 1]);
        else { std::cerr << "unknown option " << argv[a] << std::endl; return EXIT_FAILURE; }
    }
    FILE *f = std::fopen(argv[1], "rb");
    int32_t head[7], sg[11];
    double scale_cam[6], transform_to_estimate[12];
    if (!f || std::fread(head, sizeof head, 1, f) != 1 || std::fread(scale_cam, sizeof scale_cam, 1, f) != 1 ||
        std::fread(transform_to_estimate, sizeof transform_to_estimate, 1, f) != 1 || std::fread(sg, sizeof sg, 1, f) != 1 || head[0] <= 0 || head[1] <= 0 || head[2] <= 0 || head[2] > 31 ||
        head[3] < 0 || head[3] >= head[2]) {
        std::cerr << "cannot read " << argv[1] << std::endl;
        return EXIT_FAILURE;
    }
    const int rows = head[0], cols = head[1], levels = head[2], disparity_level = head[3], interpolation = head[4];
    const bool disparities_constant = head[5] != 0;
    const size_t npix = (size_t)rows * cols;
    std::vector<uint8_t> left0(npix), right0(npix), left1(npix);
    if (std::fread(left0.data(), 1, npix, f) != npix || std::fread(right0.data(), 1, npix, f) != npix || std::fread(left1.data(), 1, npix, f) != npix) {
        std::cerr << "short file " << argv[1] << std::endl;
        return EXIT_FAILURE;
    }
    std::fclose(f);
    const ceres_slam::StereoCamera camera0(scale_cam[1], scale_cam[2], scale_cam[3], scale_cam[4], scale_cam[5]);

    // Resize, compute disparity, convert, Sobel (:52-72)
    ceres_slam::StereoSGBM sgbm(sg[0], sg[1], sg[2], sg[3], sg[4], sg[5], sg[6], sg[7], sg[8], sg[9], sg[10] != 0);
    ceres_slam::ImagePyramid pyramid(left0.data(), right0.data(), left1.data(), rows, cols, levels, disparity_level, sgbm, head[6], scale_cam[0]);
    const int l = disparity_level;
    std::vector<double> &disp0 = pyramid.disparity(l);       // the blocks' memory: the matcher's map, downloaded once
    int valid = 0;
    for (double d : disp0) valid += std::isfinite(d);

    ceres::Solver::Options solver_options;
    solver_options.use_nonmonotonic_steps = true;
    if (max_iterations >= 0) solver_options.max_num_iterations = max_iterations;
    ceres::Solver::Summary summary;
    int blocks = 0;
    for (double d : disp0) blocks += std::isfinite(d) && d > 0.;

    if (coarsest >= 0) {
        std::vector<ceres::Solver::Summary> summaries;
        ceres::SolveCoarseToFine(solver_options, pyramid, camera0, transform_to_estimate, disp0.data(), coarsest, interpolation, disparities_constant,
                                 &summaries);
        for (size_t i = 0; i < summaries.size(); ++i) {
            if (summaries[i].message.empty()) std::cout << "level " << coarsest - (int)i << " " << summaries[i].BriefReport() << std::endl;
        }
        if (!summaries.empty()) summary = summaries.back();
        else summary.termination_type = ceres::FAILURE;
    } else {
        std::shared_ptr<const ceres_slam::StereoCamera> stereo_camera =
            std::make_shared<ceres_slam::StereoCamera>(ceres_slam::ImagePyramid::camera(camera0, l));
        std::shared_ptr<const ceres_slam::Image> left0_ptr = pyramid.ref(l), left1_ptr = pyramid.track(l), gradx_ptr = pyramid.gradx(l),
                                                 grady_ptr = pyramid.grady(l);
        ceres::Problem problem;
        ceres::LocalParameterization *se3_perturbation = ceres_slam::SE3Perturbation::Create();
        const int lcols = pyramid.cols(l);
        for (int v = 0; v < pyramid.rows(l); ++v) {
            double *row_ptr = &disp0[(size_t)v * lcols];
            for (int u = 0; u < lcols; ++u) {
                const double d = row_ptr[u];
                if (std::isfinite(d) && d > 0.) {
                    ceres::CostFunction *image_cost = ceres_slam::ImageError::Create(stereo_camera, left0_ptr, left1_ptr, gradx_ptr, grady_ptr,
                                                                                     (double)u, (double)v, interpolation);
                    problem.AddResidualBlock(image_cost, NULL, transform_to_estimate, row_ptr + u);
                    if (disparities_constant) problem.SetParameterBlockConstant(row_ptr + u);
                }
            }
        }
        problem.SetParameterization(transform_to_estimate, se3_perturbation);
        ceres::Solve(solver_options, &problem, &summary);
    }

    std::cout.precision(17);
    std::cout << "valid " << valid << std::endl;
    std::cout << "blocks " << blocks << std::endl;
    std::cout << "report " << summary.BriefReport() << std::endl;
    if (!summary.IsSolutionUsable()) std::cout << "message " << summary.message << std::endl;
    std::cout << "steps " << summary.num_successful_steps << " " << summary.num_unsuccessful_steps << std::endl;
    std::cout << "pose";
    for (int c = 0; c < 12; ++c) std::cout << " " << transform_to_estimate[c];
    std::cout << std::endl;
    if (!disparities_constant) {
        double sum = 0.0;
        for (double d : disp0)
            if (std::isfinite(d) && d > 0.) sum += d;
        std::cout << "disparity_sum " << sum << std::endl;
    }
    return summary.IsSolutionUsable() ? EXIT_SUCCESS : EXIT_FAILURE;
}
