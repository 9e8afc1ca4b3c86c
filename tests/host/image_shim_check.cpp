// What include/ceres_slam_amd/ceres_shim.hpp refuses of ImageError blocks (std::invalid_argument), checked on the host: every
// case throws before the first call into the back end, so no device is needed.  Prints "all refusals hold" at the end.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <limits>
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
    std::vector<double> ref = std::vector<double>(ROWS * COLS, 0.5), track = ref, gx = ref, gy = ref, other = ref;
    std::vector<double> disp = std::vector<double>(ROWS * COLS, 2.0);
    double pose[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, pose2[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::shared_ptr<const ceres_slam::Image> img(const std::vector<double> &a, int rows = ROWS, int cols = COLS) const {
        return std::make_shared<const ceres_slam::Image>(rows, cols, a.data());
    }
    ceres::CostFunction *cost(double u, double v, int interp = SSBA_IMAGE_NEAREST) const {
        return ceres_slam::ImageError::Create(camera, img(ref), img(track), img(gx), img(gy), u, v, interp);
    }
    // the driver's loop (dense_stereo_test.cpp:101-117) over the pixels with a finite positive disparity, except `skip`
    void add_all(ceres::Problem &problem, int skip = -1) {
        for (int v = 0; v < ROWS; ++v)
            for (int u = 0; u < COLS; ++u) {
                const double d = disp[v * COLS + u];
                if (v * COLS + u != skip && std::isfinite(d) && d > 0.) problem.AddResidualBlock(cost(u, v), NULL, pose, &disp[v * COLS + u]);
            }
        problem.SetParameterization(pose, ceres_slam::SE3Perturbation::Create());
    }
};

void solve(ceres::Problem &problem) {
    ceres::Solver::Options options;
    ceres::Solver::Summary summary;
    ceres::Solve(options, &problem, &summary);
}

}  // namespace

int main() {
    // ---- refused at AddResidualBlock ----
    expect_throw("a loss", "NULL loss", [] {
        Scene s; ceres::Problem p;
        std::unique_ptr<ceres::CostFunction> c(s.cost(0, 0));
        ceres::HuberLoss loss(1.0);
        p.AddResidualBlock(c.get(), &loss, s.pose, &s.disp[0]);
    });
    expect_throw("images of two sizes", "four images of one size", [] {
        Scene s; ceres::Problem p;
        std::unique_ptr<ceres::CostFunction> c(ceres_slam::ImageError::Create(s.camera, s.img(s.ref), s.img(s.track, 2, 10), s.img(s.gx), s.img(s.gy), 0, 0));
        p.AddResidualBlock(c.get(), NULL, s.pose, &s.disp[0]);
    });
    expect_throw("a pixel between positions", "integer position", [] {
        Scene s; ceres::Problem p;
        std::unique_ptr<ceres::CostFunction> c(s.cost(1.5, 0));
        p.AddResidualBlock(c.get(), NULL, s.pose, &s.disp[1]);
    });
    expect_throw("a pixel outside the image", "integer position", [] {
        Scene s; ceres::Problem p;
        std::unique_ptr<ceres::CostFunction> c(s.cost(COLS, 0));
        p.AddResidualBlock(c.get(), NULL, s.pose, &s.disp[0]);
    });
    expect_throw("another tracked image", "share their four images", [] {
        Scene s; ceres::Problem p;
        p.AddResidualBlock(s.cost(0, 0), NULL, s.pose, &s.disp[0]);
        std::unique_ptr<ceres::CostFunction> c(ceres_slam::ImageError::Create(s.camera, s.img(s.ref), s.img(s.other), s.img(s.gx), s.img(s.gy), 1, 0));
        p.AddResidualBlock(c.get(), NULL, s.pose, &s.disp[1]);
    });
    expect_throw("another interpolation", "camera and interpolation", [] {
        Scene s; ceres::Problem p;
        p.AddResidualBlock(s.cost(0, 0), NULL, s.pose, &s.disp[0]);
        std::unique_ptr<ceres::CostFunction> c(s.cost(1, 0, SSBA_IMAGE_BILINEAR));
        p.AddResidualBlock(c.get(), NULL, s.pose, &s.disp[1]);
    });
    expect_throw("another pose", "one pose block", [] {
        Scene s; ceres::Problem p;
        p.AddResidualBlock(s.cost(0, 0), NULL, s.pose, &s.disp[0]);
        std::unique_ptr<ceres::CostFunction> c(s.cost(1, 0));
        p.AddResidualBlock(c.get(), NULL, s.pose2, &s.disp[1]);
    });
    expect_throw("a disparity pointer off v * cols + u", "v * cols + u", [] {
        Scene s; ceres::Problem p;
        p.AddResidualBlock(s.cost(0, 0), NULL, s.pose, &s.disp[0]);
        std::unique_ptr<ceres::CostFunction> c(s.cost(1, 1));
        p.AddResidualBlock(c.get(), NULL, s.pose, &s.disp[1]);       // (1, 1) is element 6
    });
    // ---- refused when the problem is lowered (Solve, Covariance::Compute), before the back end is called ----
    expect_throw("some disparity blocks constant", "all disparity blocks constant or none", [] {
        Scene s; ceres::Problem p;
        s.add_all(p);
        p.SetParameterBlockConstant(&s.disp[3]);
        solve(p);
    });
    expect_throw("a usable pixel without a block", "exactly the pixels", [] {
        Scene s; ceres::Problem p;
        s.add_all(p, 7);
        solve(p);
    });
    expect_throw("a block on a pixel whose disparity is no longer usable", "exactly the pixels", [] {
        Scene s; ceres::Problem p;
        s.add_all(p);
        s.disp[7] = std::numeric_limits<double>::quiet_NaN();
        solve(p);
    });
    expect_throw("two blocks on one pixel", "two ImageError blocks", [] {
        Scene s; ceres::Problem p;
        s.add_all(p);
        p.AddResidualBlock(s.cost(2, 1), NULL, s.pose, &s.disp[7]);
        solve(p);
    });
    expect_throw("a constant pose", "cannot be held constant", [] {
        Scene s; ceres::Problem p;
        s.add_all(p);
        p.SetParameterBlockConstant(s.pose);
        solve(p);
    });
    expect_throw("a stereo block next to image blocks", "nothing else", [] {
        Scene s; ceres::Problem p;
        s.add_all(p);
        double point[3] = {0, 0, 5}, obs[3] = {2, 1.5, 0.3}, stiff[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        p.AddResidualBlock(ceres_slam::StereoReprojectionErrorAutomatic::Create(s.camera, obs, stiff), NULL, s.pose, point);
        solve(p);
    });
    expect_throw("covariance of a problem whose blocks miss a pixel", "exactly the pixels", [] {
        Scene s; ceres::Problem p;
        s.add_all(p, 0);
        ceres::Covariance::Options o;
        ceres::Covariance cov(o);
        std::vector<std::pair<const double *, const double *>> blocks(1, std::make_pair((const double *)s.pose, (const double *)s.pose));
        cov.Compute(blocks, &p);
    });
    if (failures) return EXIT_FAILURE;
    std::printf("all refusals hold\n");
    return EXIT_SUCCESS;
}
