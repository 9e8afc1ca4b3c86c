// What ceres::SolveBatch (include/ceres_slam_amd/ceres_shim.hpp) refuses with std::invalid_argument, checked on the host: every
// case throws before the first call into the back end, so no device is needed.  Prints "all refusals hold" at the end.
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "ceres_slam_amd/ceres_shim.hpp"

namespace {

const int ROWS = 4, COLS = 5;
int failures = 0;

void expect_throw(const char *what, const char *word, const std::function<void()> &f) {
    try {
        f();
    } catch (const std::invalid_argument &e) {
        if (std::string(e.what()).find(word) == std::string::npos) {
            std::printf("FAIL %s: message \"%s\" lacks \"%s\"\n", what, e.what(), word);
            ++failures;
        } else {
            std::printf("ok   %s: %s\n", what, e.what());
        }
        return;
    }
    std::printf("FAIL %s: no std::invalid_argument\n", what);
    ++failures;
}

struct Scene {
    std::shared_ptr<const ceres_slam::StereoCamera> camera = std::make_shared<ceres_slam::StereoCamera>(3.0, 3.0, 2.0, 1.5, 0.5);
    std::vector<double> img = std::vector<double>(ROWS * COLS, 0.5), disp = std::vector<double>(ROWS * COLS, 2.0);
    double pose[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    void add_all(ceres::Problem &problem) {
        std::shared_ptr<const ceres_slam::Image> i = std::make_shared<const ceres_slam::Image>(ROWS, COLS, img.data());
        for (int v = 0; v < ROWS; ++v)
            for (int u = 0; u < COLS; ++u)
                problem.AddResidualBlock(ceres_slam::ImageError::Create(camera, i, i, i, i, u, v, SSBA_IMAGE_NEAREST), NULL, pose, &disp[v * COLS + u]);
        problem.SetParameterization(pose, ceres_slam::SE3Perturbation::Create());
    }
};

}  // namespace

int main() {
    ceres::Solver::Options options;
    expect_throw("an empty vector", "no problem", [&] {
        std::vector<ceres::Solver::Summary> sums;
        ceres::SolveBatch(options, std::vector<ceres::Problem *>(), &sums);
    });
    expect_throw("a NULL entry", "is NULL", [&] {
        Scene s; ceres::Problem p; s.add_all(p);
        std::vector<ceres::Solver::Summary> sums;
        ceres::SolveBatch(options, std::vector<ceres::Problem *>{&p, nullptr}, &sums);
    });
    expect_throw("the same problem twice", "twice", [&] {
        Scene s, t; ceres::Problem p, q; s.add_all(p); t.add_all(q);
        std::vector<ceres::Solver::Summary> sums;
        ceres::SolveBatch(options, std::vector<ceres::Problem *>{&p, &q, &p}, &sums);
    });
    expect_throw("a problem with stereo blocks", "ImageError blocks and nothing else", [&] {
        Scene s; ceres::Problem p, q; s.add_all(p);
        std::shared_ptr<const ceres_slam::StereoCamera> cam = std::make_shared<ceres_slam::StereoCamera>(3.0, 3.0, 2.0, 1.5, 0.5);
        double pose[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, point[3] = {0, 0, 5}, obs[3] = {2.0, 1.5, 0.3};
        double stiffness[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        q.AddResidualBlock(ceres_slam::StereoReprojectionErrorAutomatic::Create(cam, obs, stiffness), NULL, pose, point);
        std::vector<ceres::Solver::Summary> sums;
        ceres::SolveBatch(options, std::vector<ceres::Problem *>{&p, &q}, &sums);
    });
    expect_throw("DOGLEG", "Levenberg-Marquardt only", [&] {
        Scene s; ceres::Problem p; s.add_all(p);
        ceres::Solver::Options o;
        o.trust_region_strategy_type = ceres::DOGLEG;
        std::vector<ceres::Solver::Summary> sums;
        ceres::SolveBatch(o, std::vector<ceres::Problem *>{&p}, &sums);
    });
    if (failures) { std::printf("%d refusals failed\n", failures); return 1; }
    std::printf("all refusals hold\n");
    return 0;
}
