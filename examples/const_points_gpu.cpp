// const_points_gpu -- SetParameterBlockConstant on point blocks of a stereo problem, written against
// include/ceres_slam_amd/ceres_shim.hpp: a synthetic stereo window (cameras along a line, the first one held constant, the
// others started off their true places) is solved with some or all of its map points held constant -- localisation against a
// fixed map ("all") or anchored landmarks ("third": every third point).
//
// usage: const_points_gpu [all | third [num_poses [num_points]]]
// Output (17 significant digits), so that a test can build the same problem through the C ABI and compare:
//   "problem P L N", "pose0 k <12>" and "point0 j <3>" (the initial guess), "const j" (the constant points),
//   "obs k j u v d", then "pose k <12>" and "point j <3>" (the solution) and "report <BriefReport>".
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "ceres_slam_amd/ceres_shim.hpp"

int main(int argc, char **argv) {
    const std::string which = argc > 1 ? argv[1] : "all";
    const int P = argc > 2 ? std::atoi(argv[2]) : 16;
    const int L = argc > 3 ? std::atoi(argv[3]) : 200;
    if ((which != "all" && which != "third") || P < 2 || L < 1) {
        std::cerr << "usage: const_points_gpu [all | third [num_poses >= 2 [num_points >= 1]]]" << std::endl;
        return EXIT_FAILURE;
    }
    std::shared_ptr<const ceres_slam::StereoCamera> camera = std::make_shared<ceres_slam::StereoCamera>(400.0, 400.0, 320.0, 240.0, 0.24);
    const double spacing = 0.5, reach = 2.5;          // camera k sits at x = k spacing and sees the points within `reach` of it
    std::vector<double> poses(12 * (size_t)P, 0.0), points(3 * (size_t)L), truth(3 * (size_t)L);
    for (int k = 0; k < P; ++k) {
        double *T = &poses[12 * (size_t)k];        // [t | R row-major]: q = R p + t
        T[0] = -spacing * k + (k ? 0.03 * std::sin(2.3 * k) : 0.0);      // initial guess: off the true place
        T[1] = k ? 0.02 * std::cos(1.1 * k) : 0.0;
        T[3] = T[7] = T[11] = 1.0;
    }
    for (int j = 0; j < L; ++j) {
        double *p = &truth[3 * (size_t)j];
        p[0] = -1.0 + (spacing * (P - 1) + 2.0) * (j + 0.5) / L;
        p[1] = std::sin(1.7 * j);
        p[2] = 5.0 + 3.0 * std::cos(0.9 * j);
        for (int c = 0; c < 3; ++c) points[3 * (size_t)j + c] = p[c] + 0.02 * std::sin(3.1 * j + c);
    }
    const double stiffness[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::vector<int> obs_k, obs_j;
    std::vector<double> obs_uvd;
    for (int j = 0; j < L; ++j)
        for (int k = 0; k < P; ++k) {
            const double *p = &truth[3 * (size_t)j];
            const double qx = p[0] - spacing * k, qy = p[1], qz = p[2];
            if (std::fabs(qx) > reach) continue;
            const double noise = 0.3 * std::sin(0.37 * (obs_k.size() + 1));
            obs_k.push_back(k);
            obs_j.push_back(j);
            obs_uvd.push_back(camera->fu * qx / qz + camera->cu + noise);
            obs_uvd.push_back(camera->fv * qy / qz + camera->cv - 0.5 * noise);
            obs_uvd.push_back(camera->fu * camera->b / qz + 0.1 * noise);
        }
    std::cout.precision(17);
    std::cout << "problem " << P << " " << L << " " << obs_k.size() << std::endl;
    for (int k = 0; k < P; ++k) {
        std::cout << "pose0 " << k;
        for (int c = 0; c < 12; ++c) std::cout << " " << poses[12 * (size_t)k + c];
        std::cout << std::endl;
    }
    for (int j = 0; j < L; ++j) std::cout << "point0 " << j << " " << points[3 * (size_t)j] << " " << points[3 * (size_t)j + 1] << " " << points[3 * (size_t)j + 2] << std::endl;
    for (size_t n = 0; n < obs_k.size(); ++n)
        std::cout << "obs " << obs_k[n] << " " << obs_j[n] << " " << obs_uvd[3 * n] << " " << obs_uvd[3 * n + 1] << " " << obs_uvd[3 * n + 2] << std::endl;

    ceres::Problem problem;
    ceres::LocalParameterization *se3 = ceres_slam::SE3Perturbation::Create();
    for (size_t n = 0; n < obs_k.size(); ++n)
        problem.AddResidualBlock(ceres_slam::StereoReprojectionErrorAutomatic::Create(camera, &obs_uvd[3 * n], stiffness), NULL,
                                 &poses[12 * (size_t)obs_k[n]], &points[3 * (size_t)obs_j[n]]);
    for (int k = 0; k < P; ++k) problem.SetParameterization(&poses[12 * (size_t)k], se3);
    problem.SetParameterBlockConstant(&poses[0]);
    for (int j = 0; j < L; ++j)
        if (which == "all" || j % 3 == 0) {
            problem.SetParameterBlockConstant(&points[3 * (size_t)j]);
            std::cout << "const " << j << std::endl;
        }
    ceres::Solver::Options options;
    options.max_num_iterations = 100;
    ceres::Solver::Summary summary;
    ceres::Solve(options, &problem, &summary);
    if (!summary.IsSolutionUsable()) { std::cerr << summary.message << std::endl; return EXIT_FAILURE; }
    for (int k = 0; k < P; ++k) {
        std::cout << "pose " << k;
        for (int c = 0; c < 12; ++c) std::cout << " " << poses[12 * (size_t)k + c];
        std::cout << std::endl;
    }
    for (int j = 0; j < L; ++j) std::cout << "point " << j << " " << points[3 * (size_t)j] << " " << points[3 * (size_t)j + 1] << " " << points[3 * (size_t)j + 2] << std::endl;
    std::cout << "report " << summary.BriefReport() << std::endl;
    return EXIT_SUCCESS;
}
