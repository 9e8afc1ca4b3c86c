// dense_stereo_gpu -- the reference's dense photometric driver (tests/dense_stereo_test.cpp:94-136) written against
// include/ceres_slam_amd/ceres_shim.hpp.  The reference reads a KITTI pair with OpenCV (imread, pyrDown, SGBM, Sobel: :36-72);
// this driver reads the result of that pre-processing from a raw file instead and needs no OpenCV:
//
//     int32  rows, cols, interpolation (0 nearest, 1 bilinear), disparities_constant (0 | 1)
//     double fu, fv, cu, cv, b
//     double T_track_ref[12]                 the start, [t | R row-major]
//     double disparity, ref, track, gradx, grady   rows * cols each, row-major
//
// usage: dense_stereo_gpu pair.raw [max_num_iterations] [--huber a]
// --huber a: every block carries ceres::HuberLoss(a) (the trailing argument of ImageError::Create); the covariance printed with
// constant disparities is then the one of the corrected rows.
// Output (17 significant digits): "blocks n", "report <BriefReport>", "steps <successful> <unsuccessful>", "pose <12>", and with
// free disparities "disparity_sum <sum over the blocks>", with constant ones "cov <36>" (ceres::Covariance of the pose).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <utility>
#include <vector>

#include "ceres_slam_amd/ceres_shim.hpp"

int main(int argc, char **argv) {
    if (argc < 2) {
        std::cerr << "usage: dense_stereo_gpu pair.raw [max_num_iterations] [--huber a]" << std::endl;
        return EXIT_FAILURE;
    }
    double huber_a = 0.0;
    int max_iterations = -1;
    for (int a = 2; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--huber") && a + 1 < argc) huber_a = std::atof(argv[++a]);
        else max_iterations = std::atoi(argv[a]);
    }
    FILE *f = std::fopen(argv[1], "rb");
    int32_t head[4];
    double cam[5], transform_to_estimate[12];
    if (!f || std::fread(head, sizeof head, 1, f) != 1 || std::fread(cam, sizeof cam, 1, f) != 1 ||
        std::fread(transform_to_estimate, sizeof transform_to_estimate, 1, f) != 1 || head[0] <= 0 || head[1] <= 0) {
        std::cerr << "cannot read " << argv[1] << std::endl;
        return EXIT_FAILURE;
    }
    const int rows = head[0], cols = head[1];
    const size_t npix = (size_t)rows * cols;
    std::vector<double> disp0(npix), left0(npix), left1(npix), gradx(npix), grady(npix);
    for (std::vector<double> *a : {&disp0, &left0, &left1, &gradx, &grady})
        if (std::fread(a->data(), sizeof(double), npix, f) != npix) {
            std::cerr << "short file " << argv[1] << std::endl;
            return EXIT_FAILURE;
        }
    std::fclose(f);
    std::shared_ptr<const ceres_slam::StereoCamera> stereo_camera =
        std::make_shared<ceres_slam::StereoCamera>(cam[0], cam[1], cam[2], cam[3], cam[4]);
    auto image = [&](const std::vector<double> &a) { return std::make_shared<const ceres_slam::Image>(rows, cols, a.data()); };
    std::shared_ptr<const ceres_slam::Image> left0_ptr = image(left0), left1_ptr = image(left1), gradx_ptr = image(gradx),
                                             grady_ptr = image(grady);

    ceres::Problem problem;
    ceres::LocalParameterization *se3_perturbation = ceres_slam::SE3Perturbation::Create();
    int blocks = 0;
    for (int v = 0; v < rows; ++v) {
        double *row_ptr = &disp0[(size_t)v * cols];
        for (int u = 0; u < cols; ++u) {
            const double d = row_ptr[u];
            if (std::isfinite(d) && d > 0.) {
                ceres::CostFunction *image_cost = ceres_slam::ImageError::Create(stereo_camera, left0_ptr, left1_ptr, gradx_ptr, grady_ptr,
                                                                                 (double)u, (double)v, head[2], huber_a);
                problem.AddResidualBlock(image_cost, NULL, transform_to_estimate, row_ptr + u);
                if (head[3]) problem.SetParameterBlockConstant(row_ptr + u);
                ++blocks;
            }
        }
    }
    problem.SetParameterization(transform_to_estimate, se3_perturbation);

    ceres::Solver::Options solver_options;
    solver_options.use_nonmonotonic_steps = true;
    if (max_iterations >= 0) solver_options.max_num_iterations = max_iterations;
    ceres::Solver::Summary summary;
    ceres::Solve(solver_options, &problem, &summary);

    std::cout.precision(17);
    std::cout << "blocks " << blocks << std::endl;
    std::cout << "report " << summary.BriefReport() << std::endl;
    if (!summary.IsSolutionUsable()) std::cout << "message " << summary.message << std::endl;
    std::cout << "steps " << summary.num_successful_steps << " " << summary.num_unsuccessful_steps << std::endl;
    std::cout << "pose";
    for (int c = 0; c < 12; ++c) std::cout << " " << transform_to_estimate[c];
    std::cout << std::endl;
    if (head[3]) {      // constant disparities: the covariance of the pose in tangent space (as tests/dataset_vo_sun.cpp:159-183 asks for one)
        ceres::Covariance::Options covariance_options;
        ceres::Covariance covariance(covariance_options);
        std::vector<std::pair<const double *, const double *>> covar_blocks;
        covar_blocks.push_back(std::make_pair((const double *)transform_to_estimate, (const double *)transform_to_estimate));
        double cov[36];
        if (covariance.Compute(covar_blocks, &problem) && covariance.GetCovarianceBlockInTangentSpace(transform_to_estimate, transform_to_estimate, cov)) {
            std::cout << "cov";
            for (int c = 0; c < 36; ++c) std::cout << " " << cov[c];
            std::cout << std::endl;
        } else {
            std::cout << "cov_message " << covariance.message() << std::endl;
        }
    } else {
        double sum = 0.0;
        for (size_t i = 0; i < npix; ++i)
            if (std::isfinite(disp0[i]) && disp0[i] > 0.) sum += disp0[i];
        std::cout << "disparity_sum " << sum << std::endl;
    }
    return summary.IsSolutionUsable() ? EXIT_SUCCESS : EXIT_FAILURE;
}
