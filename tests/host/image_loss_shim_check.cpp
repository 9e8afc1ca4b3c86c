// The loss of ImageError blocks in include/ceres_slam_amd/ceres_shim.hpp, checked on the host: the width is the trailing argument
// of ceres_slam::ImageError::Create, all blocks of a problem share it, and two widths in one problem throw std::invalid_argument
// at AddResidualBlock, before the first call into the back end, so no device is needed.  Prints "all loss checks hold" at the end.
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "ceres_slam_amd/ceres_shim.hpp"

namespace {

const int ROWS = 4, COLS = 5;
int failures = 0;

struct Scene {
    std::shared_ptr<const ceres_slam::StereoCamera> camera = std::make_shared<ceres_slam::StereoCamera>(3.0, 3.0, 2.0, 1.5, 0.5);
    std::vector<double> ref = std::vector<double>(ROWS * COLS, 0.5), track = ref, gx = ref, gy = ref;
    std::vector<double> disp = std::vector<double>(ROWS * COLS, 2.0);
    double pose[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::shared_ptr<const ceres_slam::Image> ir = img(ref), it = img(track), ix = img(gx), iy = img(gy);
    std::shared_ptr<const ceres_slam::Image> img(const std::vector<double> &a) const { return std::make_shared<const ceres_slam::Image>(ROWS, COLS, a.data()); }
    ceres::CostFunction *cost(int u, int v, double huber_a) const {
        return ceres_slam::ImageError::Create(camera, ir, it, ix, iy, u, v, SSBA_IMAGE_BILINEAR, huber_a);
    }
    // the driver's loop (dense_stereo_test.cpp:101-117); block `odd` gets the width `a_odd`, every other one `a`
    void add_all(ceres::Problem &problem, double a, int odd = -1, double a_odd = 0.0) {
        for (int v = 0; v < ROWS; ++v)
            for (int u = 0; u < COLS; ++u) problem.AddResidualBlock(cost(u, v, v * COLS + u == odd ? a_odd : a), NULL, pose, &disp[v * COLS + u]);
    }
};

void check(const char *what, bool ok) {
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++failures;
}

bool throws_loss_width(double a, int odd, double a_odd) {
    Scene s;
    ceres::Problem p;
    try {
        s.add_all(p, a, odd, a_odd);
    } catch (const std::invalid_argument &e) {
        std::printf("     %s\n", e.what());
        return std::string(e.what()).find("loss width") != std::string::npos;
    }
    return false;
}

}  // namespace

int main() {
    {       // Create(..., interp, 0.02) compiles and keeps the width; the default is the NULL loss; a negative width is the NULL loss
        Scene s;
        std::unique_ptr<ceres::CostFunction> c(s.cost(0, 0, 0.02)), d(ceres_slam::ImageError::Create(s.camera, s.ir, s.it, s.ix, s.iy, 0, 0)),
            e(s.cost(0, 0, -1.0));
        check("Create keeps huber_a", static_cast<ceres_slam::ImageError *>(c.get())->huber_a == 0.02);
        check("Create defaults to the NULL loss", static_cast<ceres_slam::ImageError *>(d.get())->huber_a == 0.0);
        check("a negative width is the NULL loss", static_cast<ceres_slam::ImageError *>(e.get())->huber_a == 0.0);
    }
    check("two widths in one problem throw", throws_loss_width(0.02, 7, 0.05));
    check("a block without a width among blocks with one throws", throws_loss_width(0.02, ROWS * COLS - 1, 0.0));
    check("a block with a width among blocks without one throws", throws_loss_width(0.0, 3, 0.02));
    {       // one width on every block does not throw
        Scene s;
        ceres::Problem p;
        bool ok = true;
        try { s.add_all(p, 0.02); } catch (const std::exception &e) { std::printf("     %s\n", e.what()); ok = false; }
        check("a width on every block does not throw", ok);
    }
    {       // and a loss object at AddResidualBlock is still refused: the width goes through Create
        Scene s;
        ceres::Problem p;
        std::unique_ptr<ceres::CostFunction> c(s.cost(0, 0, 0.02));
        ceres::HuberLoss loss(0.02);
        bool ok = false;
        try { p.AddResidualBlock(c.get(), &loss, s.pose, &s.disp[0]); } catch (const std::invalid_argument &e) { ok = std::string(e.what()).find("NULL loss") != std::string::npos; }
        check("AddResidualBlock with a loss object still says NULL loss", ok);
    }
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("all loss checks hold\n");
    return 0;
}
