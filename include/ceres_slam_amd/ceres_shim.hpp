// ceres_shim.hpp -- header-only C++11 shim that reproduces, on top of the C ABI in
// include/ssba.h, the call shapes the ceres-slam stereo drivers use against Ceres
// (/root/reference tests/dataset_vo.cpp:22-85):
//
//     ceres::Problem problem;
//     ceres::LocalParameterization *se3 = ceres_slam::SE3Perturbation::Create();
//     ceres::CostFunction *cost = ceres_slam::StereoReprojectionErrorAutomatic::Create(camera, obs, stiffness);
//     problem.AddResidualBlock(cost, NULL, pose_k, point_j);
//     problem.SetParameterization(pose_k, se3);
//     problem.SetParameterBlockConstant(pose_0);
//     ceres::Solver::Options options;  options.max_num_iterations = 1000; ...
//     ceres::Solver::Summary summary;  ceres::Solve(options, &problem, &summary);
//     std::cout << summary.BriefReport();
//
// and of the Phong driver (tests/dataset_ba_phong.cpp:26-255):
//
//     problem.AddResidualBlock(IntensityErrorPointLightAutomatic::Create(I, int_stiffness), NULL,
//                              pose_k, position_j, normal_j, phong_m, texture_m, light);
//     problem.AddResidualBlock(NormalErrorAutomatic::Create(n_obs, normal_stiffness), NULL, pose_k, normal_j);
//     problem.SetParameterization(normal_j, unit_vector_perturbation);
//     problem.SetParameterLowerBound(phong_m, 0, 0.);  problem.SetParameterUpperBound(phong_m, 0, 1.); ...
//     options.trust_region_strategy_type = ceres::DOGLEG;  options.dogleg_type = ceres::SUBSPACE_DOGLEG;
//
// and of the sun-aided VO driver (tests/dataset_vo_sun.cpp:28-185):
//
//     problem.AddResidualBlock(StereoReprojectionErrorAutomatic::Create(camera, obs, stiffness_of_point_j), NULL, pose_k, point_j);
//     problem.AddResidualBlock(SunSensorErrorAutomatic::Create(sun_obs_c, sun_dir_g, stiffness2x2, az_thresh, zen_thresh),
//                              new ceres::HuberLoss(huber_param), pose_k);
//     problem.AddResidualBlock(PoseErrorAutomatic::Create(T_ref, stiffness6x6), NULL, pose_k1);
//     ceres::Covariance covariance(covariance_options);
//     covariance.Compute(covar_blocks, &problem);
//     covariance.GetCovarianceBlockInTangentSpace(pose, pose, out36);     // (pose | point, pose | point) pairs
//
// and of the dense photometric driver (tests/dense_stereo_test.cpp:94-136), with ceres_slam::Image in place of cv::Mat:
//
//     problem.AddResidualBlock(ceres_slam::ImageError::Create(camera, ref, track, gradx, grady, u, v), NULL, pose, &disparity[v * cols + u]);
//     problem.SetParameterization(pose, se3_perturbation);
//
// The shim recognises the typed cost functions of this path and lowers them to observation
// tables; it does NOT run arbitrary user functors on the GPU -- any other CostFunction is
// rejected at AddResidualBlock with std::invalid_argument (Ceres would accept it: that is the
// documented limit of the drop-in).  Parameter blocks stay caller-owned; identity = address.
// Eigen is not needed: observations and stiffness are plain arrays.
#ifndef CERES_SLAM_AMD_CERES_SHIM_HPP_
#define CERES_SLAM_AMD_CERES_SHIM_HPP_

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../ssba.h"

namespace ceres {

class CostFunction { public: virtual ~CostFunction() {} };
class LocalParameterization { public: virtual ~LocalParameterization() {} };
class LossFunction { public: virtual ~LossFunction() {} };
class HuberLoss : public LossFunction {
 public:
    explicit HuberLoss(double a) : a_(a) {}
    double a() const { return a_; }
 private:
    double a_;
};

enum TerminationType { CONVERGENCE = 0, NO_CONVERGENCE = 1, FAILURE = 2 };
enum LinearSolverType { SPARSE_NORMAL_CHOLESKY, SPARSE_SCHUR, DENSE_SCHUR };
enum TrustRegionStrategyType { LEVENBERG_MARQUARDT, DOGLEG };
enum DoglegType { TRADITIONAL_DOGLEG, SUBSPACE_DOGLEG };
enum CovarianceAlgorithmType { DENSE_SVD, SPARSE_QR };
enum SparseLinearAlgebraLibraryType { SUITE_SPARSE, CX_SPARSE, EIGEN_SPARSE, NO_SPARSE };

}  // namespace ceres

namespace ceres_slam {

// include/ceres_slam/stereo_camera.hpp:159-163
struct StereoCamera {
    double fu, fv, cu, cv, b;
    StereoCamera(double fu_, double fv_, double cu_, double cv_, double b_) : fu(fu_), fv(fv_), cu(cu_), cv(cv_), b(b_) {}
};

// include/ceres_slam/stereo_reprojection_error.hpp:59-69
class StereoReprojectionErrorAutomatic : public ceres::CostFunction {
 public:
    static ceres::CostFunction *Create(const std::shared_ptr<const StereoCamera> &camera, const double observation[3],
                                       const double stiffness[9]) {
        StereoReprojectionErrorAutomatic *c = new StereoReprojectionErrorAutomatic;
        c->camera = camera;
        std::memcpy(c->observation, observation, sizeof c->observation);
        std::memcpy(c->stiffness, stiffness, sizeof c->stiffness);
        return c;
    }
    std::shared_ptr<const StereoCamera> camera;
    double observation[3];
    double stiffness[9];
};

// include/ceres_slam/pose_error.hpp:59-66: prior on a pose block, r = S log(T_ref T^-1); T_ref is the 12-double
// [t | R row-major] block (SE3Group::data()), stiffness 6x6 row-major
class PoseErrorAutomatic : public ceres::CostFunction {
 public:
    static ceres::CostFunction *Create(const double T_k_0_ref[12], const double stiffness[36]) {
        PoseErrorAutomatic *c = new PoseErrorAutomatic;
        std::memcpy(c->T_ref, T_k_0_ref, sizeof c->T_ref);
        std::memcpy(c->stiffness, stiffness, sizeof c->stiffness);
        return c;
    }
    double T_ref[12], stiffness[36];
};

// include/ceres_slam/relative_pose_error.hpp:46-57: measurement T_2_1_ref between two pose blocks, r = S log(T_ref T_1 T_2^-1)
class RelativePoseErrorAutomatic : public ceres::CostFunction {
 public:
    static ceres::CostFunction *Create(const double T_2_1_ref[12], const double stiffness[36]) {
        RelativePoseErrorAutomatic *c = new RelativePoseErrorAutomatic;
        std::memcpy(c->T_ref, T_2_1_ref, sizeof c->T_ref);
        std::memcpy(c->stiffness, stiffness, sizeof c->stiffness);
        return c;
    }
    double T_ref[12], stiffness[36];
};

// include/ceres_slam/sun_sensor_error.hpp:108-120: azimuth / zenith error of the expected sun direction, stiffness 2x2
class SunSensorErrorAutomatic : public ceres::CostFunction {
 public:
    static ceres::CostFunction *Create(const double observed_sun_dir_c[3], const double expected_sun_dir_g[3], const double stiffness[4],
                                       double az_err_thresh, double zen_err_thresh) {
        SunSensorErrorAutomatic *c = new SunSensorErrorAutomatic;
        std::memcpy(c->observed, observed_sun_dir_c, sizeof c->observed);
        std::memcpy(c->expected, expected_sun_dir_g, sizeof c->expected);
        std::memcpy(c->stiffness, stiffness, sizeof c->stiffness);
        c->az_thresh = az_err_thresh;
        c->zen_thresh = zen_err_thresh;
        return c;
    }
    double observed[3], expected[3], stiffness[4], az_thresh, zen_thresh;
};

// include/ceres_slam/perturbations.hpp:69-75
class SE3Perturbation : public ceres::LocalParameterization {
 public:
    static ceres::LocalParameterization *Create() { return new SE3Perturbation; }
};

// include/ceres_slam/perturbations.hpp:87-113
class UnitVectorPerturbation : public ceres::LocalParameterization {
 public:
    static ceres::LocalParameterization *Create() { return new UnitVectorPerturbation; }
};

// include/ceres_slam/intensity_error_point_light.hpp:98-112 / intensity_error_directional_light.hpp:98-113:
// blocks (pose 12, position 3, normal 3, Phong parameters 3, texture 1, light 3) -> 1 residual
class IntensityErrorAutomaticBase : public ceres::CostFunction {
 public:
    double colour = 0.0, stiffness = 0.0;
    int light_type = 0;      // 0 point light, 1 directional light
};
class IntensityErrorPointLightAutomatic : public IntensityErrorAutomaticBase {
 public:
    static ceres::CostFunction *Create(double colour, double stiffness) {
        IntensityErrorPointLightAutomatic *c = new IntensityErrorPointLightAutomatic;
        c->colour = colour; c->stiffness = stiffness; c->light_type = 0;
        return c;
    }
};
class IntensityErrorDirectionalLightAutomatic : public IntensityErrorAutomaticBase {
 public:
    static ceres::CostFunction *Create(double colour, double stiffness) {
        IntensityErrorDirectionalLightAutomatic *c = new IntensityErrorDirectionalLightAutomatic;
        c->colour = colour; c->stiffness = stiffness; c->light_type = 1;
        return c;
    }
};

// include/ceres_slam/normal_error.hpp:46-54: blocks (pose 12, normal 3) -> 3 residuals
class NormalErrorAutomatic : public ceres::CostFunction {
 public:
    static ceres::CostFunction *Create(const double obs[3], const double stiffness[9]) {
        NormalErrorAutomatic *c = new NormalErrorAutomatic;
        std::memcpy(c->obs, obs, sizeof c->obs);
        std::memcpy(c->stiffness, stiffness, sizeof c->stiffness);
        return c;
    }
    double obs[3];
    double stiffness[9];
};

// A row-major image of doubles: what the dense driver holds in cv::Mat (CV_64F) after its OpenCV pre-processing
struct Image {
    int rows, cols;
    const double *data;
    Image(int rows_, int cols_, const double *data_) : rows(rows_), cols(cols_), data(data_) {}
    // an image handed out by ImagePyramid is also one of the four device images (which: 0 ref, 1 track, 2 gradx, 3 grady) of a level
    ssba_image_pyramid *pyramid = nullptr;
    int level = -1, which = -1;
};

// A row-major 8-bit image: what the dense driver holds in cv::Mat (CV_8U) after imread and pyrDown
struct Image8 {
    int rows, cols;
    const uint8_t *data;
    Image8(int rows_, int cols_, const uint8_t *data_) : rows(rows_), cols(cols_), data(data_) {}
};

// What cv::StereoSGBM writes (disp16: CV_16S, sixteenths of a pixel, (minDisparity - 1) * 16 at invalid pixels) and what the
// driver's disp0.convertTo(disp0, CV_64F, 1. / 16.) makes of it, with NaN instead of minDisparity - 1 at invalid pixels
struct DisparityMap {
    int rows = 0, cols = 0;
    std::vector<int16_t> disp16;
    std::vector<double> disparity;
};

// cv::StereoSGBM in the call shape of the dense driver (tests/dense_stereo_test.cpp:61-65):
//     ceres_slam::StereoSGBM sgbm(0, 64, 15);  sgbm(left0, right0, disp0);
// The semi-global matcher of ssba_stereo_sgbm (include/ssba.h states its arithmetic; bit parity with OpenCV is unpinned).
// std::invalid_argument where the C call refuses (images of different sizes included), std::runtime_error for every other failure.
class StereoSGBM {
 public:
    StereoSGBM(int minDisparity = 0, int numDisparities = 64, int SADWindowSize = 15, int P1 = 0, int P2 = 0, int disp12MaxDiff = 0, int preFilterCap = 0,
               int uniquenessRatio = 0, int speckleWindowSize = 0, int speckleRange = 0, bool fullDP = false, int device_ = -1)
        : device(device_) {
        ssba_sgbm_default_params(&params);
        params.min_disparity = minDisparity; params.num_disparities = numDisparities; params.block_size = SADWindowSize;
        params.p1 = P1; params.p2 = P2; params.disp12_max_diff = disp12MaxDiff; params.pre_filter_cap = preFilterCap;
        params.uniqueness_ratio = uniquenessRatio; params.speckle_window_size = speckleWindowSize; params.speckle_range = speckleRange;
        params.full_dp = fullDP ? 1 : 0;
    }
    void operator()(const Image8 &left, const Image8 &right, DisparityMap &disp) const {
        if (left.rows != right.rows || left.cols != right.cols || left.rows <= 0 || left.cols <= 0)
            throw std::invalid_argument("ceres_shim: StereoSGBM needs two images of one size");
        const size_t npix = (size_t)left.rows * (size_t)left.cols;
        disp.rows = left.rows; disp.cols = left.cols;
        disp.disp16.assign(npix, 0);
        disp.disparity.assign(npix, 0.0);
        Raise("ssba_stereo_sgbm", ssba_stereo_sgbm(left.data, right.data, (uint32_t)left.rows, (uint32_t)left.cols, &params, device, disp.disp16.data(),
                                                   disp.disparity.data()));
    }
    // n pairs of one size in shared launches (ssba_stereo_sgbm_batch): disp[k] is bit-equal to (*this)(left[k], right[k], disp[k]).
    // workspace_bytes bounds the matcher's volumes (0: the library's 1 GiB); the pairs run in chunks of as many as fit.
    void operator()(const std::vector<Image8> &left, const std::vector<Image8> &right, std::vector<DisparityMap> &disp, uint64_t workspace_bytes = 0) const {
        if (left.size() != right.size()) throw std::invalid_argument("ceres_shim: StereoSGBM needs as many left images as right images");
        const size_t n = left.size();
        const int rows = n ? left[0].rows : 0, cols = n ? left[0].cols : 0;
        for (size_t k = 0; k < n; ++k)
            if (left[k].rows != rows || left[k].cols != cols || right[k].rows != rows || right[k].cols != cols || rows <= 0 || cols <= 0)
                throw std::invalid_argument("ceres_shim: StereoSGBM needs pairs of one size");
        const size_t npix = (size_t)rows * (size_t)cols;
        std::vector<uint8_t> L(n * npix), R(n * npix);
        for (size_t k = 0; k < n; ++k) {
            std::memcpy(L.data() + k * npix, left[k].data, npix);
            std::memcpy(R.data() + k * npix, right[k].data, npix);
        }
        std::vector<int16_t> d16(n * npix);
        std::vector<double> d(n * npix);
        Raise("ssba_stereo_sgbm_batch", ssba_stereo_sgbm_batch(L.data(), R.data(), (uint32_t)n, (uint32_t)rows, (uint32_t)cols, &params, workspace_bytes, device,
                                                               d16.data(), d.data()));
        disp.resize(n);
        for (size_t k = 0; k < n; ++k) {
            disp[k].rows = rows; disp[k].cols = cols;
            disp[k].disp16.assign(d16.begin() + (std::ptrdiff_t)(k * npix), d16.begin() + (std::ptrdiff_t)((k + 1) * npix));
            disp[k].disparity.assign(d.begin() + (std::ptrdiff_t)(k * npix), d.begin() + (std::ptrdiff_t)((k + 1) * npix));
        }
    }
    static void Raise(const char *call, int rc) {
        if (!rc) return;
        const std::string msg = std::string(call) + ": " + ssba_status_string(rc) + " (" + ssba_last_error() + ")";
        if (rc == SSBA_ERR_INVALID_ARGUMENT || rc == SSBA_ERR_UNSUPPORTED) throw std::invalid_argument(msg);
        throw std::runtime_error(msg);
    }
    ssba_sgbm_params params;
    int device;
};

// The pre-processing of the dense driver (tests/dense_stereo_test.cpp:52-72: pyrDown, convertTo, Sobel) on the device, in place of
// the cv::Mat the driver holds per level: built once from the raw 8-bit pair and the disparity map of ONE level
// (ssba_image_pyramid_create), it hands out std::shared_ptr<const Image> per level.  The images are backed by the device level;
// their host copy (Image::data) is filled EAGERLY, in the constructor, so every image behaves like a caller-made one.  When the
// four images of ImageError::Create are the ref / track / gradx / grady of one level, the problem binds the level with
// ssba_add_image_level and nothing is uploaded from the host.  The images keep the pyramid alive.
class ImagePyramid {
 public:
    ImagePyramid(const uint8_t *ref_u8, const uint8_t *track_u8, const double *disparity, int rows, int cols, int levels, int disparity_level,
                 int gradient_source = SSBA_GRADIENT_OF_REFERENCE, double gradient_scale = 1.0, int device = -1)
        : s_(std::make_shared<State>()) {
        int rc = ssba_image_pyramid_create(ref_u8, track_u8, disparity, (uint32_t)rows, (uint32_t)cols, (uint32_t)levels, (uint32_t)disparity_level,
                                           gradient_source, gradient_scale, device, &s_->h);
        if (rc) throw std::runtime_error(std::string("ssba_image_pyramid_create: ") + ssba_status_string(rc) + " (" + ssba_last_error() + ")");
        Download(rows, cols, levels, disparity_level);
    }
    // From what the rig delivers (ssba_image_pyramid_create_stereo): the right image of the reference instant instead of a disparity
    // map; `matcher` runs on the device at disparity_level, where the driver calls SGBM (:52-64), and disparity(level) is its map.
    // std::invalid_argument where the C call refuses.
    ImagePyramid(const uint8_t *ref_left_u8, const uint8_t *ref_right_u8, const uint8_t *track_u8, int rows, int cols, int levels, int disparity_level,
                 const StereoSGBM &matcher, int gradient_source = SSBA_GRADIENT_OF_REFERENCE, double gradient_scale = 1.0, int device = -1)
        : s_(std::make_shared<State>()) {
        StereoSGBM::Raise("ssba_image_pyramid_create_stereo",
                          ssba_image_pyramid_create_stereo(ref_left_u8, ref_right_u8, track_u8, (uint32_t)rows, (uint32_t)cols, (uint32_t)levels,
                                                           (uint32_t)disparity_level, &matcher.params, gradient_source, gradient_scale, device, &s_->h));
        Download(rows, cols, levels, disparity_level);
    }
    int levels() const { return (int)s_->lv.size(); }
    int disparity_level() const { return s_->disparity_level; }
    int rows(int level) const { return s_->lv.at((size_t)level).img[0].rows; }
    int cols(int level) const { return s_->lv.at((size_t)level).img[0].cols; }
    std::shared_ptr<const Image> image(int level, int which) const {
        return std::shared_ptr<const Image>(s_, &s_->lv.at((size_t)level).img.at((size_t)which));
    }
    std::shared_ptr<const Image> ref(int level) const { return image(level, 0); }
    std::shared_ptr<const Image> track(int level) const { return image(level, 1); }
    std::shared_ptr<const Image> gradx(int level) const { return image(level, 2); }
    std::shared_ptr<const Image> grady(int level) const { return image(level, 3); }
    // the host copy of a level's disparity map (levels >= disparity_level): memory for the disparity blocks of that level
    std::vector<double> &disparity(int level) {
        if (level < s_->disparity_level) throw std::invalid_argument("ceres_shim: levels finer than disparity_level have no disparity map");
        return s_->lv.at((size_t)level).disparity;
    }
    // fu, fv, cu, cv over 2^level, b unchanged (pyrDown samples at even pixels)
    static StereoCamera camera(const StereoCamera &level0, int level) {
        const double s = std::ldexp(1.0, -level);
        return StereoCamera(level0.fu * s, level0.fv * s, level0.cu * s, level0.cv * s, level0.b);
    }
    ssba_image_pyramid *handle() const { return s_->h; }
    // the ceres::HuberLoss(a) of every level's blocks in both SolveCoarseToFine overloads (ssba_image_pyramid_set_huber_loss);
    // a <= 0: the NULL loss again
    void SetHuberLoss(double a) {
        const int rc = ssba_image_pyramid_set_huber_loss(s_->h, a);
        if (rc) throw std::runtime_error(std::string("ssba_image_pyramid_set_huber_loss: ") + ssba_status_string(rc) + " (" + ssba_last_error() + ")");
    }

 private:
    friend class ImageSequence;
    // a pyramid borrowed from an image sequence (ssba_image_sequence_pyramid): never destroyed here, and `owner` keeps the sequence alive
    ImagePyramid(ssba_image_pyramid *borrowed, const std::shared_ptr<void> &owner, int rows, int cols, int levels, int disparity_level)
        : s_(std::make_shared<State>()) {
        s_->h = borrowed;
        s_->borrowed = true;
        s_->owner = owner;
        Download(rows, cols, levels, disparity_level);
    }
    struct Level;
    void Download(int rows, int cols, int levels, int disparity_level) {
        s_->disparity_level = disparity_level;
        s_->lv.resize((size_t)levels);
        for (int l = 0; l < levels; ++l) {
            Level &L = s_->lv[(size_t)l];
            const size_t npix = (size_t)(rows >> l) * (size_t)(cols >> l);
            for (int q = 0; q < 4; ++q) L.host[q].resize(npix);
            if (l >= disparity_level) L.disparity.resize(npix);
            uint32_t r = 0, c = 0;
            const int rc = ssba_image_pyramid_level(s_->h, (uint32_t)l, &r, &c, NULL, NULL, L.host[0].data(), L.host[1].data(), L.host[2].data(), L.host[3].data(),
                                          l >= disparity_level ? L.disparity.data() : NULL);
            if (rc) throw std::runtime_error(std::string("ssba_image_pyramid_level: ") + ssba_status_string(rc) + " (" + ssba_last_error() + ")");
            for (int q = 0; q < 4; ++q) {
                L.img.push_back(Image((int)r, (int)c, L.host[q].data()));
                L.img.back().pyramid = s_->h; L.img.back().level = l; L.img.back().which = q;
            }
        }
    }
    struct Level {
        std::vector<double> host[4], disparity;
        std::vector<Image> img;
    };
    struct State {
        ssba_image_pyramid *h = nullptr;
        int disparity_level = 0;
        std::vector<Level> lv;
        bool borrowed = false;
        std::shared_ptr<void> owner;       // released after the body of ~State
        ~State() { if (h && !borrowed) ssba_image_pyramid_destroy(h); }
    };
    std::shared_ptr<State> s_;
};

// A rectified stereo sequence prepared once (ssba_image_sequence_create): F left frames and the right frames 0 ... F - 2, each stack
// contiguous, rows * cols bytes per frame.  Every frame is uploaded once, every left frame's levels, double image and gradients are
// built once, and `matcher` runs over the F - 1 pairs (left_k, right_k) in shared launches.  pyramid(k) is the ImagePyramid of pair k
// (reference frame k, tracked frame k + 1), bit-equal to ImagePyramid(left_k, right_k, left_(k+1), ..., matcher, ...); it is borrowed
// from the sequence, and it and its images keep the sequence alive.  std::invalid_argument where the C call refuses.
class ImageSequence {
 public:
    ImageSequence(const uint8_t *left, const uint8_t *right, int frames, int rows, int cols, int levels, int disparity_level, const StereoSGBM &matcher,
                  int gradient_source = SSBA_GRADIENT_OF_REFERENCE, double gradient_scale = 1.0, uint64_t workspace_bytes = 0, int device = -1)
        : s_(std::make_shared<State>()) {
        Create(left, right, frames, rows, cols, levels, disparity_level, matcher, gradient_source, gradient_scale, workspace_bytes, device);
    }
    // the same from one pointer per frame: right may hold F or F - 1 images
    ImageSequence(const std::vector<const uint8_t *> &left, const std::vector<const uint8_t *> &right, int rows, int cols, int levels, int disparity_level,
                  const StereoSGBM &matcher, int gradient_source = SSBA_GRADIENT_OF_REFERENCE, double gradient_scale = 1.0, uint64_t workspace_bytes = 0,
                  int device = -1)
        : s_(std::make_shared<State>()) {
        if (left.size() < 2 || (right.size() != left.size() && right.size() + 1 != left.size()) || rows <= 0 || cols <= 0)
            throw std::invalid_argument("ceres_shim: ImageSequence needs F >= 2 left frames and F or F - 1 right frames of one size");
        const size_t npix = (size_t)rows * (size_t)cols, F = left.size();
        std::vector<uint8_t> L(F * npix), R((F - 1) * npix);
        for (size_t k = 0; k < F; ++k) {
            if (!left[k] || (k + 1 < F && !right[k])) throw std::invalid_argument("ceres_shim: ImageSequence: NULL frame");
            std::memcpy(L.data() + k * npix, left[k], npix);
            if (k + 1 < F) std::memcpy(R.data() + k * npix, right[k], npix);
        }
        Create(L.data(), R.data(), (int)F, rows, cols, levels, disparity_level, matcher, gradient_source, gradient_scale, workspace_bytes, device);
    }
    int pairs() const { return (int)s_->pyramids.size(); }
    ImagePyramid &pyramid(int k) {
        if (k < 0 || k >= pairs()) throw std::invalid_argument("ceres_shim: ImageSequence: no such pair");
        return *s_->pyramids[(size_t)k];
    }
    std::vector<ImagePyramid *> pyramids() {
        std::vector<ImagePyramid *> out;
        for (std::unique_ptr<ImagePyramid> &p : s_->pyramids) out.push_back(p.get());
        return out;
    }

 private:
    struct Handle {
        ssba_image_sequence *h = nullptr;
        ~Handle() { if (h) ssba_image_sequence_destroy(h); }
    };
    struct State {
        std::shared_ptr<Handle> seq;
        std::vector<std::unique_ptr<ImagePyramid>> pyramids;
    };
    void Create(const uint8_t *left, const uint8_t *right, int frames, int rows, int cols, int levels, int disparity_level, const StereoSGBM &matcher,
                int gradient_source, double gradient_scale, uint64_t workspace_bytes, int device) {
        s_->seq = std::make_shared<Handle>();
        StereoSGBM::Raise("ssba_image_sequence_create",
                          ssba_image_sequence_create(left, right, (uint32_t)frames, (uint32_t)rows, (uint32_t)cols, (uint32_t)levels, (uint32_t)disparity_level,
                                                     &matcher.params, workspace_bytes, gradient_source, gradient_scale, device, &s_->seq->h));
        for (int k = 0; k + 1 < frames; ++k) {
            ssba_image_pyramid *h = nullptr;
            StereoSGBM::Raise("ssba_image_sequence_pyramid", ssba_image_sequence_pyramid(s_->seq->h, (uint32_t)k, &h));
            s_->pyramids.emplace_back(new ImagePyramid(h, s_->seq, rows, cols, levels, disparity_level));
        }
    }
    std::shared_ptr<State> s_;
};

// include/ceres_slam/image_error.hpp:136-144: blocks (pose 12 = T_track_ref, disparity 1) -> 1 residual at reference pixel (u, v).
// interpolation: SSBA_IMAGE_NEAREST is the functor as it stands (:156-164), SSBA_IMAGE_BILINEAR what its comment announces.
// huber_a > 0 is the width of the ceres::HuberLoss(huber_a) a caller would hand to AddResidualBlock (ssba_set_huber_loss on the
// image handle); AddResidualBlock itself still takes a NULL loss for these blocks, and all blocks of a problem share one width.
class ImageError : public ceres::CostFunction {
 public:
    static ceres::CostFunction *Create(const std::shared_ptr<const StereoCamera> &camera, const std::shared_ptr<const Image> &ref_img,
                                       const std::shared_ptr<const Image> &track_img, const std::shared_ptr<const Image> &track_gradx,
                                       const std::shared_ptr<const Image> &track_grady, double u_ref, double v_ref,
                                       int interpolation = SSBA_IMAGE_NEAREST, double huber_a = 0.0) {
        ImageError *c = new ImageError;
        c->camera = camera;
        c->img[0] = ref_img; c->img[1] = track_img; c->img[2] = track_gradx; c->img[3] = track_grady;
        c->u = u_ref; c->v = v_ref; c->interpolation = interpolation;
        c->huber_a = huber_a > 0.0 ? huber_a : 0.0;
        return c;
    }
    std::shared_ptr<const StereoCamera> camera;
    std::shared_ptr<const Image> img[4];
    double u, v;
    int interpolation;
    double huber_a = 0.0;
};

}  // namespace ceres_slam

namespace ceres {

class Problem;

class Solver {
 public:
    // the Options fields the drivers set (tests/dataset_vo.cpp:65-74), Ceres 1.x defaults
    struct Options {
        bool minimizer_progress_to_stdout = false;
        int num_threads = 1;
        int num_linear_solver_threads = 1;
        int max_num_iterations = 50;
        bool use_nonmonotonic_steps = false;
        TrustRegionStrategyType trust_region_strategy_type = LEVENBERG_MARQUARDT;
        DoglegType dogleg_type = TRADITIONAL_DOGLEG;
        LinearSolverType linear_solver_type = SPARSE_SCHUR;
        double function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
        double initial_trust_region_radius = 1e4;
    };
    struct Summary {
        TerminationType termination_type = NO_CONVERGENCE;
        int num_successful_steps = 0, num_unsuccessful_steps = 0;
        int num_line_search_steps = 0;      // bounds: evaluations of the projected line search (device + host)
        double initial_cost = 0, final_cost = 0, total_time_in_seconds = 0;
        std::string message;
        bool IsSolutionUsable() const { return termination_type == CONVERGENCE || termination_type == NO_CONVERGENCE; }
        std::string BriefReport() const {
            ssba_summary s;
            std::memset(&s, 0, sizeof s);
            s.termination_type = termination_type;
            s.num_successful_steps = num_successful_steps;
            s.num_unsuccessful_steps = num_unsuccessful_steps;
            s.initial_cost = initial_cost;
            s.final_cost = final_cost;
            char buf[256];
            ssba_brief_report(&s, buf, sizeof buf);
            return buf;
        }
    };
};

class Problem {
 public:
    Problem() {}
    ~Problem() {   // Ceres default: the problem owns cost functions, losses, parameterisations
        for (auto c : owned_costs_) delete c;
        for (auto &kv : owned_losses_) delete kv.first;
        for (auto &kv : owned_params_) delete kv.first;
        if (h_) ssba_destroy(h_);
    }
    Problem(const Problem &) = delete;
    Problem &operator=(const Problem &) = delete;

    // intensity residual block (tests/dataset_ba_phong.cpp:108-139)
    void AddResidualBlock(CostFunction *cost, LossFunction *loss, double *pose_block, double *position_block, double *normal_block,
                          double *phong_block, double *texture_block, double *light_block) {
        ++version_;
        auto *c = dynamic_cast<ceres_slam::IntensityErrorAutomaticBase *>(cost);
        if (!c) throw std::invalid_argument("ceres_shim: a six-block residual must be an IntensityError*Automatic");
        if (loss) throw std::invalid_argument("ceres_shim: lighting residual blocks take a NULL loss");
        if (!intensity_.empty() && (c->stiffness != intensity_[0].stiffness || c->light_type != intensity_[0].light_type ||
                                    light_block != light_))
            throw std::invalid_argument("ceres_shim: intensity residual blocks must share stiffness, light type and light block");
        light_ = light_block;
        IntensityBlock b;
        b.pose = pose_block; b.position = position_block; b.normal = normal_block; b.phong = phong_block; b.texture = texture_block;
        b.colour = c->colour; b.stiffness = c->stiffness; b.light_type = c->light_type;
        intensity_.push_back(b);
        owned_costs_.push_back(cost);
    }

    // unary pose residual blocks (tests/dataset_vo_sun.cpp:80-124): pose prior, sun sensor (optionally with HuberLoss)
    void AddResidualBlock(CostFunction *cost, LossFunction *loss, double *pose_block) {
        ++version_;
        PoseFactor f;
        std::memset(&f, 0, sizeof f);
        if (auto *c = dynamic_cast<ceres_slam::PoseErrorAutomatic *>(cost)) {
            f.type = 0;
            std::memcpy(f.data, c->T_ref, sizeof c->T_ref);
            std::memcpy(f.stiffness, c->stiffness, sizeof c->stiffness);
        } else if (auto *c2 = dynamic_cast<ceres_slam::SunSensorErrorAutomatic *>(cost)) {
            f.type = 1;
            std::memcpy(f.data, c2->observed, sizeof c2->observed);
            std::memcpy(f.data + 3, c2->expected, sizeof c2->expected);
            f.data[6] = c2->az_thresh; f.data[7] = c2->zen_thresh;
            std::memcpy(f.stiffness, c2->stiffness, sizeof c2->stiffness);
        } else {
            throw std::invalid_argument("ceres_shim: a one-block residual must be a PoseErrorAutomatic or SunSensorErrorAutomatic");
        }
        if (loss) {
            HuberLoss *h = dynamic_cast<HuberLoss *>(loss);
            if (!h) throw std::invalid_argument("ceres_shim: loss must be NULL or ceres::HuberLoss");
            owned_losses_[loss] = 1;
            f.huber = h->a();
        }
        f.pose = pose_block;
        block_index(pose_index_, pose_blocks_, pose_block);
        pose_factors_.push_back(f);
        owned_costs_.push_back(cost);
    }

    void AddResidualBlock(CostFunction *cost, LossFunction *loss, double *pose_block, double *point_block) {
        ++version_;
        if (auto *im = dynamic_cast<ceres_slam::ImageError *>(cost)) {      // (pose, disparity): dense_stereo_test.cpp:106-112
            add_image_block_(im, loss, pose_block, point_block);
            owned_costs_.push_back(cost);
            return;
        }
        if (auto *rp = dynamic_cast<ceres_slam::RelativePoseErrorAutomatic *>(cost)) {      // (pose 1, pose 2): blowup_test.cpp:70-76
            RelFactor f;
            std::memset(&f, 0, sizeof f);
            f.pose1 = pose_block; f.pose2 = point_block;
            std::memcpy(f.T_ref, rp->T_ref, sizeof f.T_ref);
            std::memcpy(f.stiffness, rp->stiffness, sizeof f.stiffness);
            if (loss) {
                HuberLoss *h = dynamic_cast<HuberLoss *>(loss);
                if (!h) throw std::invalid_argument("ceres_shim: loss must be NULL or ceres::HuberLoss");
                owned_losses_[loss] = 1;
                f.huber = h->a();
            }
            block_index(pose_index_, pose_blocks_, pose_block);
            block_index(pose_index_, pose_blocks_, point_block);
            rel_factors_.push_back(f);
            owned_costs_.push_back(cost);
            return;
        }
        if (auto *n = dynamic_cast<ceres_slam::NormalErrorAutomatic *>(cost)) {   // (pose, normal): dataset_ba_phong.cpp:181-188
            if (loss) throw std::invalid_argument("ceres_shim: lighting residual blocks take a NULL loss");
            NormalBlock b;
            b.pose = pose_block; b.normal = point_block;
            std::memcpy(b.obs, n->obs, sizeof b.obs);
            std::memcpy(b.stiffness, n->stiffness, sizeof b.stiffness);
            normals_.push_back(b);
            owned_costs_.push_back(cost);
            return;
        }
        auto *s = dynamic_cast<ceres_slam::StereoReprojectionErrorAutomatic *>(cost);
        if (!s) throw std::invalid_argument("ceres_shim: only StereoReprojectionErrorAutomatic residual blocks run on the GPU path");
        const HuberLoss *h = nullptr;
        if (loss) {
            h = dynamic_cast<HuberLoss *>(loss);
            if (!h) throw std::invalid_argument("ceres_shim: loss must be NULL or ceres::HuberLoss");
            owned_losses_[loss] = 1;
        }
        const double a = h ? h->a() : 0.0;
        if (obs_pose_.empty()) {
            camera_ = s->camera;
            huber_a_ = a;
        } else if (a != huber_a_ ||
                   (s->camera != camera_ && std::memcmp(s->camera.get(), camera_.get(), sizeof(ceres_slam::StereoCamera)) != 0)) {
            throw std::invalid_argument("ceres_shim: all stereo residual blocks must share camera and loss");
        }
        obs_stiffness_.insert(obs_stiffness_.end(), s->stiffness, s->stiffness + 9);    // may differ per block (dataset_vo_sun.cpp:56-65)
        obs_pose_.push_back(block_index(pose_index_, pose_blocks_, pose_block));
        obs_point_.push_back(block_index(point_index_, point_blocks_, point_block));
        obs_uvd_.insert(obs_uvd_.end(), s->observation, s->observation + 3);
        owned_costs_.push_back(cost);
    }
    // Ceres: Problem::AddParameterBlock(values, size, local_parameterization).  Registers a pose block (size 12) or a
    // point block (size 3) ahead of its residual blocks.  Sharded runs (SetDistributed) need it for the poses: every rank
    // must hold every pose, in the same order, also where it owns no observation of it.
    void AddParameterBlock(double *values, int size, LocalParameterization *lp = nullptr) {
        ++version_;
        if (size == 12) block_index(pose_index_, pose_blocks_, values);
        else if (size == 3) block_index(point_index_, point_blocks_, values);
        else throw std::invalid_argument("ceres_shim: AddParameterBlock takes pose (12) or point (3) blocks");
        if (lp) SetParameterization(values, lp);
    }
    // Extension (not in Ceres): this problem is one shard of a landmark-sharded problem -- rank `rank` of `world_size`
    // processes, one per GPU; the shards' reduced camera systems are summed by ncclAllReduce inside libssba.so
    // (ssba_set_distributed + ssba_set_rccl; the 128-byte id comes from ssba_rccl_unique_id on rank 0).  Every rank adds all
    // pose blocks (AddParameterBlock) and the residual blocks of its own landmarks; Solve is then a collective call.
    void SetDistributed(int world_size, int rank, const void *rccl_unique_id) {
        ++version_;
        dist_world_ = world_size; dist_rank_ = rank;
        std::memcpy(dist_id_, rccl_unique_id, sizeof dist_id_);
    }
    void SetParameterization(double *block, LocalParameterization *lp) {
        owned_params_[lp] = 1;
        if (dynamic_cast<ceres_slam::UnitVectorPerturbation *>(lp)) { unit_vector_[block] = 1; return; }   // normals, light direction
        if (!dynamic_cast<ceres_slam::SE3Perturbation *>(lp)) throw std::invalid_argument("ceres_shim: only SE3Perturbation / UnitVectorPerturbation are supported");
        if (!pose_index_.count(block)) throw std::invalid_argument("ceres_shim: parameter block not found");
        parameterized_[block] = 1;
    }
    // poses: per block; shared lighting blocks (light, Phong parameters, textures): checked at Solve, the
    // GPU path holds ALL blocks of one kind constant or none (what the driver's DEBUG lines do)
    // point (position) blocks: any subset on a stereo problem; with lighting residuals all or none (stage 2 of --multistage)
    void SetParameterBlockConstant(double *block) { if (!constant_.count(block)) { constant_[block] = 1; ++version_; } }
    void SetParameterBlockVariable(double *block) { if (constant_.erase(block)) ++version_; }
    void SetParameterLowerBound(double *block, int index, double v) { lower_[block][index] = v; ++version_; }
    void SetParameterUpperBound(double *block, int index, double v) { upper_[block][index] = v; ++version_; }
    int NumResidualBlocks() const { return (int)(obs_pose_.size() + image_blocks_.size()); }

 private:
    friend void Solve(const Solver::Options &, Problem *, Solver::Summary *);
    friend void SolveBatch(const Solver::Options &, const std::vector<Problem *> &, std::vector<Solver::Summary> *);
    friend const char *shim_prepare(Problem &, int *);
    friend class Covariance;
    // back-end handle of the current structure and the contiguous staging tables it points into
    ssba_problem *h_ = nullptr;
    unsigned long version_ = 0, h_version_ = ~0ul;
    std::vector<double> st_poses_, st_points_, st_normals_, st_phong_, st_texture_, st_intensity_, st_normal_obs_;
    std::vector<double *> normal_blocks_, phong_blocks_, texture_blocks_;
    std::vector<uint32_t> st_material_of_point_;
    double st_light_[3] = {0, 0, 0};
    // the stereo + unary-pose part of the lowering, shared by Solve and Covariance::Compute; returns the failing call or NULL
    const char *lower_core_(ssba_problem *h, std::vector<double> &poses, std::vector<double> &points, int *rc) {
        if ((*rc = ssba_add_pose_blocks(h, poses.data(), (uint32_t)pose_blocks_.size()))) return "ssba_add_pose_blocks";
        if ((*rc = ssba_add_point_blocks(h, points.data(), (uint32_t)point_blocks_.size()))) return "ssba_add_point_blocks";
        for (size_t b = 0; b < obs_pose_.size();) {      // runs of equal stiffness: one call each (a single run for the other drivers)
            size_t e = b + 1;
            while (e < obs_pose_.size() && std::memcmp(&obs_stiffness_[9 * e], &obs_stiffness_[9 * b], 9 * sizeof(double)) == 0) ++e;
            if ((*rc = ssba_add_stereo_observations(h, &obs_pose_[b], &obs_point_[b], &obs_uvd_[3 * b], e - b, &obs_stiffness_[9 * b])))
                return "ssba_add_stereo_observations";
            b = e;
        }
        for (auto &kv : constant_)
            if (pose_index_.count(kv.first) && (*rc = ssba_set_pose_constant(h, pose_index_[kv.first], 1))) return "ssba_set_pose_constant";
        // position blocks: with lighting residuals all constant (stage 2 of --multistage, dataset_ba_phong.cpp:213-220) or none;
        // a stereo problem holds any subset (ssba_set_point_constant)
        std::vector<uint32_t> const_points;
        for (size_t j = 0; j < point_blocks_.size(); ++j)
            if (constant_.count(point_blocks_[j])) const_points.push_back((uint32_t)j);
        if (const_points.size() == point_blocks_.size() || !intensity_.empty()) {
            if (!const_points.empty() && const_points.size() != point_blocks_.size())
                throw std::invalid_argument("ceres_shim: with lighting residuals hold all point blocks constant or none");
            if (!const_points.empty() && (*rc = ssba_set_point_blocks_constant(h, 1))) return "ssba_set_point_blocks_constant";
        } else if (!const_points.empty() && (*rc = ssba_set_point_constant(h, const_points.data(), const_points.size(), 1))) {
            return "ssba_set_point_constant";
        }
        for (auto &f : pose_factors_) {
            const uint32_t k = pose_index_[f.pose];
            if (f.type == 0) { if ((*rc = ssba_add_pose_prior(h, k, f.data, f.stiffness, f.huber))) return "ssba_add_pose_prior"; }
            else if ((*rc = ssba_add_sun_observation(h, k, f.data, f.data + 3, f.stiffness, f.data[6], f.data[7], f.huber))) return "ssba_add_sun_observation";
        }
        for (auto &f : rel_factors_)
            if ((*rc = ssba_add_relative_pose(h, pose_index_[f.pose1], pose_index_[f.pose2], f.T_ref, f.stiffness, f.huber))) return "ssba_add_relative_pose";
        if (huber_a_ > 0 && (*rc = ssba_set_huber_loss(h, huber_a_))) return "ssba_set_huber_loss";
        return nullptr;
    }
    // ImageError blocks: the back end takes them as one disparity MAP (ssba_add_image_blocks), so all blocks share the camera, the
    // four images, the interpolation and the pose, and the disparity block of pixel (u, v) is element v * cols + u of one array
    void add_image_block_(ceres_slam::ImageError *im, LossFunction *loss, double *pose, double *disparity) {
        if (loss) throw std::invalid_argument("ceres_shim: ImageError residual blocks take a NULL loss");
        if (!im->camera) throw std::invalid_argument("ceres_shim: ImageError needs a camera");
        for (int q = 0; q < 4; ++q)
            if (!im->img[q] || !im->img[q]->data || im->img[q]->rows != im->img[0]->rows || im->img[q]->cols != im->img[0]->cols || im->img[0]->rows <= 0 || im->img[0]->cols <= 0)
                throw std::invalid_argument("ceres_shim: ImageError needs four images of one size");
        const int rows = im->img[0]->rows, cols = im->img[0]->cols;
        const long u = (long)im->u, v = (long)im->v;
        if ((double)u != im->u || (double)v != im->v || u < 0 || v < 0 || u >= cols || v >= rows)
            throw std::invalid_argument("ceres_shim: ImageError reference pixel must be an integer position inside the image");
        double *base = disparity - ((size_t)v * cols + (size_t)u);
        if (image_blocks_.empty()) {
            image_first_ = *im;
            image_pose_ = pose;
            image_disp_ = base;
        } else {
            for (int q = 0; q < 4; ++q)
                if (im->img[q]->data != image_first_.img[q]->data) throw std::invalid_argument("ceres_shim: all ImageError blocks must share their four images");
            if (rows != image_first_.img[0]->rows || cols != image_first_.img[0]->cols || im->interpolation != image_first_.interpolation ||
                std::memcmp(im->camera.get(), image_first_.camera.get(), sizeof(ceres_slam::StereoCamera)) != 0)
                throw std::invalid_argument("ceres_shim: all ImageError blocks must share image size, camera and interpolation");
            if (im->huber_a != image_first_.huber_a) throw std::invalid_argument("ceres_shim: all ImageError blocks must share one loss width (huber_a)");
            if (pose != image_pose_) throw std::invalid_argument("ceres_shim: all ImageError blocks must share one pose block");
            if (base != image_disp_)
                throw std::invalid_argument("ceres_shim: the disparity block of ImageError pixel (u, v) must be element v * cols + u of one rows * cols array");
        }
        block_index(pose_index_, pose_blocks_, pose);
        image_blocks_.push_back((uint32_t)((size_t)v * cols + (size_t)u));
    }
    ceres_slam::ImageError image_first_;
    double *image_pose_ = nullptr, *image_disp_ = nullptr;
    std::vector<uint32_t> image_blocks_;         // pixel of every ImageError block
    static uint32_t block_index(std::map<double *, uint32_t> &idx, std::vector<double *> &blocks, double *b) {
        auto it = idx.find(b);
        if (it != idx.end()) return it->second;
        const uint32_t i = (uint32_t)blocks.size();
        idx[b] = i;
        blocks.push_back(b);
        return i;
    }
    std::shared_ptr<const ceres_slam::StereoCamera> camera_;
    std::vector<double> obs_stiffness_;          // 9 per stereo residual block
    double huber_a_ = 0.0;
    struct PoseFactor { int type; double *pose; double data[18], stiffness[36], huber; };
    std::vector<PoseFactor> pose_factors_;
    struct RelFactor { double *pose1, *pose2; double T_ref[12], stiffness[36], huber; };
    std::vector<RelFactor> rel_factors_;
    std::map<double *, uint32_t> pose_index_, point_index_;
    int dist_world_ = 0, dist_rank_ = 0;
    unsigned char dist_id_[SSBA_RCCL_UNIQUE_ID_BYTES];
    std::vector<double *> pose_blocks_, point_blocks_;
    std::vector<uint32_t> obs_pose_, obs_point_;
    std::vector<double> obs_uvd_;
    std::map<double *, int> parameterized_, constant_, unit_vector_;
    struct IntensityBlock { double *pose, *position, *normal, *phong, *texture; double colour, stiffness; int light_type; };
    struct NormalBlock { double *pose, *normal; double obs[3], stiffness[9]; };
    std::vector<IntensityBlock> intensity_;
    std::vector<NormalBlock> normals_;
    double *light_ = nullptr;
    std::map<double *, std::map<int, double>> lower_, upper_;
    std::vector<CostFunction *> owned_costs_;
    std::map<LossFunction *, int> owned_losses_;
    std::map<LocalParameterization *, int> owned_params_;
};

// Gathers the caller's blocks into the problem's contiguous staging tables (the C ABI takes block tables) and makes
// sure a finalized handle for the problem's CURRENT structure exists: built on first use, kept across Solve /
// Covariance::Compute calls, rebuilt after any AddResidualBlock / SetParameterBlock* / bound change.  Returns the
// failing call (status in *rc) or NULL.
inline const char *shim_prepare(Problem &P, int *rc_out) {
    int &rc = *rc_out;
    rc = 0;
    for (double *b : P.pose_blocks_)
        if (!P.parameterized_.count(b)) throw std::invalid_argument("ceres_shim: pose block without SE3Perturbation");
    std::vector<double> &poses = P.st_poses_, &points = P.st_points_;
    poses.resize(P.pose_blocks_.size() * 12);
    points.resize(P.point_blocks_.size() * 3);
    for (size_t i = 0; i < P.pose_blocks_.size(); ++i) std::memcpy(&poses[12 * i], P.pose_blocks_[i], 12 * sizeof(double));
    for (size_t i = 0; i < P.point_blocks_.size(); ++i) std::memcpy(&points[3 * i], P.point_blocks_[i], 3 * sizeof(double));
    std::vector<double> &normals = P.st_normals_, &phong = P.st_phong_, &texture = P.st_texture_, &intensity = P.st_intensity_,
                        &normal_obs = P.st_normal_obs_;
    std::vector<double *> &normal_blocks = P.normal_blocks_, &phong_blocks = P.phong_blocks_, &texture_blocks = P.texture_blocks_;
    std::vector<uint32_t> &material_of_point = P.st_material_of_point_;
    double (&light)[3] = P.st_light_;
    const bool lighting = !P.intensity_.empty();
    if (!P.image_blocks_.empty() && !(P.h_ && P.h_version_ == P.version_)) {
        // ---- ImageError blocks (tests/dense_stereo_test.cpp:101-117) -> ssba_add_image_blocks on the caller's own pose and map ----
        if (!P.obs_pose_.empty() || !P.pose_factors_.empty() || !P.rel_factors_.empty() || lighting || !P.normals_.empty() || P.dist_world_ > 0 ||
            P.pose_blocks_.size() != 1 || !P.point_blocks_.empty())
            throw std::invalid_argument("ceres_shim: a problem with ImageError blocks holds one pose, its disparity blocks and nothing else");
        if (P.constant_.count(P.image_pose_)) throw std::invalid_argument("ceres_shim: the pose of ImageError blocks cannot be held constant");
        const ceres_slam::ImageError &f = P.image_first_;
        const size_t npix = (size_t)f.img[0]->rows * f.img[0]->cols;
        // the back end builds a block for every pixel whose disparity is finite and positive (:105): the caller's set must be that one
        std::vector<unsigned char> has(npix, 0);
        size_t n_const = 0;
        for (uint32_t pix : P.image_blocks_) {
            if (has[pix]) throw std::invalid_argument("ceres_shim: two ImageError blocks on one pixel");
            has[pix] = 1;
            n_const += P.constant_.count(P.image_disp_ + pix);
        }
        for (size_t i = 0; i < npix; ++i) {
            const double dd = P.image_disp_[i];
            if ((dd == dd && dd - dd == 0.0 && dd > 0.0) != (has[i] != 0))
                throw std::invalid_argument("ceres_shim: ImageError blocks must cover exactly the pixels with a finite positive disparity");
        }
        if (n_const != 0 && n_const != P.image_blocks_.size()) throw std::invalid_argument("ceres_shim: hold all disparity blocks constant or none");
        if (P.h_) { ssba_destroy(P.h_); P.h_ = nullptr; }
        ssba_camera cam = ssba_camera{f.camera->fu, f.camera->fv, f.camera->cu, f.camera->cv, f.camera->b};
        if ((rc = ssba_create(&cam, -1, &P.h_))) { P.h_ = nullptr; return "ssba_create"; }
        const char *where = nullptr;
        // ref, track, gradx, grady of ONE pyramid level: the level is bound on the device, nothing is uploaded from the host
        bool one_level = f.img[0]->pyramid != nullptr;
        for (int q = 0; q < 4; ++q) one_level = one_level && f.img[q]->pyramid == f.img[0]->pyramid && f.img[q]->level == f.img[0]->level && f.img[q]->which == q;
        if (one_level) {
            if ((rc = ssba_add_image_level(P.h_, f.img[0]->pyramid, (uint32_t)f.img[0]->level, P.image_pose_, P.image_disp_, f.interpolation)))
                where = "ssba_add_image_level";
        } else if ((rc = ssba_add_image_blocks(P.h_, P.image_pose_, P.image_disp_, f.img[0]->data, f.img[1]->data, f.img[2]->data, f.img[3]->data,
                                        (uint32_t)f.img[0]->rows, (uint32_t)f.img[0]->cols, f.interpolation))) where = "ssba_add_image_blocks";
        if (where) {}
        else if (f.huber_a > 0.0 && (rc = ssba_set_huber_loss(P.h_, f.huber_a))) where = "ssba_set_huber_loss";
        else if (n_const && (rc = ssba_set_disparity_blocks_constant(P.h_, 1))) where = "ssba_set_disparity_blocks_constant";
        else if ((rc = ssba_finalize(P.h_))) where = "ssba_finalize";
        if (where) { ssba_destroy(P.h_); P.h_ = nullptr; return where; }
        P.h_version_ = P.version_;
        return nullptr;
    }
    if (P.h_ && P.h_version_ == P.version_) {      // same structure: only the values may have moved
        if (lighting) {
            for (size_t j = 0; j < P.point_blocks_.size(); ++j) std::memcpy(&normals[3 * j], normal_blocks[j], 3 * sizeof(double));
            for (size_t m = 0; m < phong_blocks.size(); ++m) { std::memcpy(&phong[3 * m], phong_blocks[m], 3 * sizeof(double)); texture[m] = *texture_blocks[m]; }
            std::memcpy(light, P.light_, sizeof light);
        }
        return nullptr;
    }
    if (P.h_) { ssba_destroy(P.h_); P.h_ = nullptr; }
    ssba_camera cam = {1.0, 1.0, 0.0, 0.0, 1.0};      // pose-graph problems (tests/blowup_test.cpp) have no stereo block
    if (P.camera_) cam = ssba_camera{P.camera_->fu, P.camera_->fv, P.camera_->cu, P.camera_->cv, P.camera_->b};
    ssba_problem *&h = P.h_;
    rc = ssba_create(&cam, -1, &h);
    auto fail = [&](const char *where) -> const char * {
        if (h) { ssba_destroy(h); h = nullptr; }
        return where;
    };
    if (rc) return fail("ssba_create");
    if (P.dist_world_ > 0 && (rc = ssba_set_distributed(h, P.dist_world_, P.dist_rank_))) return fail("ssba_set_distributed");
    if (const char *where = P.lower_core_(h, poses, points, &rc)) return fail(where);
    // ---- lighting terms (tests/dataset_ba_phong.cpp:101-204) -> the config-3 tables of the C ABI ----
    normal_blocks.assign(P.point_blocks_.size(), nullptr);
    phong_blocks.clear();
    texture_blocks.clear();
    material_of_point.assign(P.point_blocks_.size(), 0);
    if (lighting) {
        const size_t N = P.obs_pose_.size();
        if (P.intensity_.size() != N || P.normals_.size() != N)
            throw std::invalid_argument("ceres_shim: every stereo observation needs one intensity and one normal residual block");
        std::map<std::pair<double *, double *>, size_t> obs_of;      // (pose, position) -> stereo observation
        for (size_t i = 0; i < N; ++i) obs_of[{P.pose_blocks_[P.obs_pose_[i]], P.point_blocks_[P.obs_point_[i]]}] = i;
        std::map<double *, uint32_t> material_index, point_of_normal;
        intensity.assign(N, 0.0);
        normal_obs.assign(3 * N, 0.0);
        for (auto &b : P.intensity_) {
            auto it = obs_of.find({b.pose, b.position});
            if (it == obs_of.end()) throw std::invalid_argument("ceres_shim: intensity residual without a stereo residual on the same (pose, point)");
            const uint32_t j = P.point_index_[b.position];
            if (normal_blocks[j] && normal_blocks[j] != b.normal) throw std::invalid_argument("ceres_shim: a vertex has two normal blocks");
            normal_blocks[j] = b.normal;
            point_of_normal[b.normal] = j;
            if (!material_index.count(b.phong)) {
                material_index[b.phong] = (uint32_t)phong_blocks.size();
                phong_blocks.push_back(b.phong);
                texture_blocks.push_back(b.texture);
            }
            const uint32_t m = material_index[b.phong];
            if (texture_blocks[m] != b.texture) throw std::invalid_argument("ceres_shim: Phong parameter and texture blocks must pair one-to-one");
            material_of_point[j] = m;
            intensity[it->second] = b.colour;
        }
        for (auto &b : P.normals_) {
            auto pj = point_of_normal.find(b.normal);
            if (pj == point_of_normal.end()) throw std::invalid_argument("ceres_shim: normal residual on an unknown normal block");
            auto it = obs_of.find({b.pose, P.point_blocks_[pj->second]});
            if (it == obs_of.end()) throw std::invalid_argument("ceres_shim: normal residual without a stereo residual on the same (pose, point)");
            std::memcpy(&normal_obs[3 * it->second], b.obs, 3 * sizeof(double));
            if (std::memcmp(b.stiffness, P.normals_[0].stiffness, sizeof b.stiffness) != 0)
                throw std::invalid_argument("ceres_shim: normal residual blocks must share their stiffness");
        }
        const size_t M = phong_blocks.size();
        normals.resize(3 * P.point_blocks_.size());
        for (size_t j = 0; j < P.point_blocks_.size(); ++j) {
            if (!normal_blocks[j]) throw std::invalid_argument("ceres_shim: a vertex without lighting terms");
            if (!P.unit_vector_.count(normal_blocks[j])) throw std::invalid_argument("ceres_shim: normal block without UnitVectorPerturbation");
            std::memcpy(&normals[3 * j], normal_blocks[j], 3 * sizeof(double));
        }
        phong.resize(3 * M); texture.resize(M);
        for (size_t m = 0; m < M; ++m) { std::memcpy(&phong[3 * m], phong_blocks[m], 3 * sizeof(double)); texture[m] = *texture_blocks[m]; }
        std::memcpy(light, P.light_, sizeof light);
        const int light_type = P.intensity_[0].light_type;
        if (light_type == 1 && !P.unit_vector_.count(P.light_)) throw std::invalid_argument("ceres_shim: light direction without UnitVectorPerturbation");
        if ((rc = ssba_add_normal_blocks(h, normals.data(), (uint32_t)P.point_blocks_.size()))) return fail("ssba_add_normal_blocks");
        if ((rc = ssba_add_material_blocks(h, phong.data(), texture.data(), (uint32_t)M, material_of_point.data(), (uint32_t)P.point_blocks_.size())))
            return fail("ssba_add_material_blocks");
        if ((rc = ssba_add_light_block(h, light, light_type))) return fail("ssba_add_light_block");
        if ((rc = ssba_add_lighting_observations(h, intensity.data(), P.intensity_[0].stiffness, normal_obs.data(), P.normals_[0].stiffness, N)))
            return fail("ssba_add_lighting_observations");
        // SetParameterBlockConstant / bounds on shared blocks: all blocks of a kind or none
        auto all_or_none = [&](const std::vector<double *> &blocks, const char *what) {
            size_t n = 0;
            for (double *b : blocks) n += P.constant_.count(b);
            if (n != 0 && n != blocks.size()) throw std::invalid_argument(std::string("ceres_shim: hold all ") + what + " blocks constant or none");
            return n != 0;
        };
        if ((rc = ssba_set_shared_block_constant(h, SSBA_BLOCK_LIGHT, P.constant_.count(P.light_) ? 1 : 0))) return fail("ssba_set_shared_block_constant");
        if ((rc = ssba_set_shared_block_constant(h, SSBA_BLOCK_PHONG, all_or_none(phong_blocks, "Phong parameter") ? 1 : 0))) return fail("ssba_set_shared_block_constant");
        if ((rc = ssba_set_shared_block_constant(h, SSBA_BLOCK_TEXTURE, all_or_none(texture_blocks, "texture") ? 1 : 0))) return fail("ssba_set_shared_block_constant");
        auto bounds = [&](const std::vector<double *> &blocks, int which, int size) -> int {
            for (int idx = 0; idx < size; ++idx) {
                auto get = [&](std::map<double *, std::map<int, double>> &tab, double *b, double none) {
                    auto it = tab.find(b);
                    if (it == tab.end() || !it->second.count(idx)) return none;
                    return it->second[idx];
                };
                const double inf = 1.0 / 0.0;
                const double lo = get(P.lower_, blocks[0], -inf), hi = get(P.upper_, blocks[0], inf);
                for (double *b : blocks)
                    if (get(P.lower_, b, -inf) != lo || get(P.upper_, b, inf) != hi)
                        throw std::invalid_argument("ceres_shim: bounds must be the same on all blocks of a kind");
                if (lo != -inf || hi != inf)
                    if (int r = ssba_set_shared_block_bounds(h, which, idx, lo, hi)) return r;
            }
            return 0;
        };
        if ((rc = bounds(phong_blocks, SSBA_BLOCK_PHONG, 3))) return fail("ssba_set_shared_block_bounds");
        if ((rc = bounds(texture_blocks, SSBA_BLOCK_TEXTURE, 1))) return fail("ssba_set_shared_block_bounds");
    }
    if ((rc = ssba_finalize(h))) return fail("ssba_finalize");
    if (P.dist_world_ > 0 && (rc = ssba_set_rccl(h, P.dist_id_, sizeof P.dist_id_))) return fail("ssba_set_rccl");
    P.h_version_ = P.version_;
    return nullptr;
}

inline ssba_options shim_options(const Solver::Options &options) {
    ssba_options o;
    ssba_default_options(&o);
    o.max_num_iterations = options.max_num_iterations;
    o.use_nonmonotonic_steps = options.use_nonmonotonic_steps ? 1 : 0;
    o.minimizer_progress_to_stdout = options.minimizer_progress_to_stdout ? 1 : 0;
    o.num_threads = options.num_threads;
    o.num_linear_solver_threads = options.num_linear_solver_threads;
    o.function_tolerance = options.function_tolerance;
    o.gradient_tolerance = options.gradient_tolerance;
    o.parameter_tolerance = options.parameter_tolerance;
    o.initial_trust_region_radius = options.initial_trust_region_radius;
    o.trust_region_strategy_type = options.trust_region_strategy_type == DOGLEG ? 1 : 0;
    o.dogleg_type = options.dogleg_type == SUBSPACE_DOGLEG ? 1 : 0;
    return o;
}
inline void shim_summary(const ssba_summary &s, Solver::Summary *summary) {
    summary->termination_type = (TerminationType)s.termination_type;
    summary->num_successful_steps = s.num_successful_steps;
    summary->num_unsuccessful_steps = s.num_unsuccessful_steps;
    summary->num_line_search_steps = s.num_line_search_steps;
    summary->initial_cost = s.initial_cost;
    summary->final_cost = s.final_cost;
    summary->total_time_in_seconds = s.total_time_s;
}

// Coarse to fine on an image pyramid (ssba_image_pyramid_align): one Levenberg-Marquardt solve per level from coarsest_level down
// to the pyramid's disparity_level, the pose carried along.  level0_camera is the camera of level 0; pose (12) and disparity (the
// map at disparity_level, e.g. pyramid.disparity(pyramid.disparity_level())) are updated in place.  summaries gets one entry per
// level solved, coarsest first; a call that fails outright leaves one FAILURE entry with the message.
inline void SolveCoarseToFine(const Solver::Options &options, ceres_slam::ImagePyramid &pyramid, const ceres_slam::StereoCamera &level0_camera,
                              double *pose, double *disparity, int coarsest_level, int interpolation, bool disparities_constant,
                              std::vector<Solver::Summary> *summaries) {
    const ssba_options o = shim_options(options);
    const ssba_camera cam = ssba_camera{level0_camera.fu, level0_camera.fv, level0_camera.cu, level0_camera.cv, level0_camera.b};
    const int n = std::max(coarsest_level - pyramid.disparity_level() + 1, 1);
    std::vector<ssba_summary> s((size_t)n);
    std::memset(s.data(), 0, s.size() * sizeof(ssba_summary));
    for (ssba_summary &x : s) x.termination_type = -1;
    const int rc = ssba_image_pyramid_align(pyramid.handle(), &cam, pose, disparity, (uint32_t)coarsest_level, interpolation, disparities_constant ? 1 : 0,
                                            &o, s.data());
    summaries->clear();
    for (const ssba_summary &x : s) {
        if (x.termination_type < 0) break;      // levels the loop did not reach
        summaries->push_back(Solver::Summary());
        shim_summary(x, &summaries->back());
    }
    if (rc && rc != SSBA_ERR_NUMERICAL_FAILURE) {
        summaries->push_back(Solver::Summary());
        summaries->back().termination_type = FAILURE;
        summaries->back().message = std::string("ssba_image_pyramid_align: ") + ssba_status_string(rc) + " (" + ssba_last_error() + ")";
    }
}

// Coarse to fine over several pyramids in lockstep (ssba_image_pyramid_align_batch): the pairs of a sequence, one shared solve per
// level.  poses holds 12 doubles per pyramid, disparities one map at disparity_level per pyramid; both are updated in place.
// summaries gets one vector per pyramid (the levels solved, coarsest first); a pyramid that ends a level without a usable solution
// keeps its last usable pose and its last entry says FAILURE.  Throws std::invalid_argument where the C call refuses.
inline void SolveCoarseToFine(const Solver::Options &options, const std::vector<ceres_slam::ImagePyramid *> &pyramids,
                              const ceres_slam::StereoCamera &level0_camera, double *poses, const std::vector<double *> &disparities,
                              int coarsest_level, int interpolation, bool disparities_constant,
                              std::vector<std::vector<Solver::Summary>> *summaries) {
    if (pyramids.size() != disparities.size()) throw std::invalid_argument("ceres_shim: SolveCoarseToFine needs one disparity map per pyramid");
    const ssba_options o = shim_options(options);
    const ssba_camera cam = ssba_camera{level0_camera.fu, level0_camera.fv, level0_camera.cu, level0_camera.cv, level0_camera.b};
    std::vector<ssba_image_pyramid *> hs;
    for (ceres_slam::ImagePyramid *p : pyramids) hs.push_back(p ? p->handle() : nullptr);
    const int levels = pyramids.empty() || !pyramids[0] ? 1 : std::max(coarsest_level - pyramids[0]->disparity_level() + 1, 1);
    std::vector<ssba_summary> s(std::max<size_t>(pyramids.size(), 1) * (size_t)levels);
    std::vector<int> st(std::max<size_t>(pyramids.size(), 1), 0);
    std::vector<double *> maps(disparities);
    if (maps.empty()) maps.push_back(nullptr);
    if (hs.empty()) hs.push_back(nullptr);
    const int rc = ssba_image_pyramid_align_batch(hs.data(), (uint32_t)pyramids.size(), &cam, poses, maps.data(), (uint32_t)coarsest_level, interpolation,
                                                  disparities_constant ? 1 : 0, &o, s.data(), st.data());
    bool member = false;
    for (size_t k = 0; k < pyramids.size(); ++k) member = member || st[k] != 0;
    if (rc && !member) {
        const std::string msg = std::string("ssba_image_pyramid_align_batch: ") + ssba_status_string(rc) + " (" + ssba_last_error() + ")";
        if (rc == SSBA_ERR_INVALID_ARGUMENT || rc == SSBA_ERR_UNSUPPORTED || rc == SSBA_ERR_STATE) throw std::invalid_argument(msg);
        throw std::runtime_error(msg);
    }
    summaries->assign(pyramids.size(), std::vector<Solver::Summary>());
    for (size_t k = 0; k < pyramids.size(); ++k) {
        for (int l = 0; l < levels; ++l) {
            const ssba_summary &x = s[k * (size_t)levels + (size_t)l];
            if (x.num_iterations == 0) break;      // levels this pyramid did not reach
            (*summaries)[k].push_back(Solver::Summary());
            shim_summary(x, &(*summaries)[k].back());
        }
        if (st[k] && st[k] != SSBA_ERR_NUMERICAL_FAILURE) {
            (*summaries)[k].push_back(Solver::Summary());
            (*summaries)[k].back().termination_type = FAILURE;
            (*summaries)[k].back().message = std::string("ssba_image_pyramid_align_batch: ") + ssba_status_string(st[k]);
        }
    }
}

// ceres::Solve(options, &problem, &summary) (tests/dataset_vo.cpp:81).  Never throws for
// solver outcomes: the result is in `summary` (as with Ceres); API misuse throws.
inline void Solve(const Solver::Options &options, Problem *problem, Solver::Summary *summary) {
    Problem &P = *problem;
    *summary = Solver::Summary();
    if (P.obs_pose_.empty() && P.pose_factors_.empty() && P.rel_factors_.empty() && P.image_blocks_.empty() && P.dist_world_ <= 1) {     // (a shard without blocks still joins the collectives)
        summary->termination_type = CONVERGENCE;
        summary->message = "no residual blocks";
        return;
    }
    int rc = 0;
    auto fail = [&](const char *where) {
        summary->termination_type = FAILURE;
        summary->message = std::string(where) + ": " + ssba_status_string(rc) + " (" + ssba_last_error() + ")";
    };
    if (const char *where = shim_prepare(P, &rc)) return fail(where);
    ssba_problem *h = P.h_;
    std::vector<double> &poses = P.st_poses_, &points = P.st_points_, &normals = P.st_normals_, &phong = P.st_phong_, &texture = P.st_texture_;
    std::vector<double *> &normal_blocks = P.normal_blocks_, &phong_blocks = P.phong_blocks_, &texture_blocks = P.texture_blocks_;
    double (&light)[3] = P.st_light_;
    const bool lighting = !P.intensity_.empty();
    const ssba_options o = shim_options(options);
    ssba_summary s;
    rc = ssba_solve(h, &o, &s);
    if (rc && rc != SSBA_ERR_NUMERICAL_FAILURE) return fail("ssba_solve");
    shim_summary(s, summary);
    if (summary->IsSolutionUsable() && P.image_blocks_.empty()) {      // (ImageError blocks: the back end wrote the caller's pose and map itself)
        for (size_t i = 0; i < P.pose_blocks_.size(); ++i) std::memcpy(P.pose_blocks_[i], &poses[12 * i], 12 * sizeof(double));
        for (size_t i = 0; i < P.point_blocks_.size(); ++i) std::memcpy(P.point_blocks_[i], &points[3 * i], 3 * sizeof(double));
        if (lighting) {   // every lighting block is written back; constant ones come back unchanged
            for (size_t j = 0; j < P.point_blocks_.size(); ++j) std::memcpy(normal_blocks[j], &normals[3 * j], 3 * sizeof(double));
            for (size_t m = 0; m < phong_blocks.size(); ++m) { std::memcpy(phong_blocks[m], &phong[3 * m], 3 * sizeof(double)); *texture_blocks[m] = texture[m]; }
            std::memcpy(P.light_, light, sizeof light);
        }
    }
}

// Several problems that hold only ImageError blocks, solved in shared launches (ssba_image_solve_batch): every summary is what
// ceres::Solve would have given for that problem alone, and the callers' poses and disparity maps are written as there.  A problem
// whose minimiser fails does not stop the others.  Throws std::invalid_argument where the C call refuses: an empty vector, a NULL
// entry, the same problem twice, a problem with other blocks than ImageError, DOGLEG.
inline void SolveBatch(const Solver::Options &options, const std::vector<Problem *> &problems, std::vector<Solver::Summary> *summaries) {
    if (problems.empty()) throw std::invalid_argument("ceres_shim: SolveBatch: no problem");
    for (size_t k = 0; k < problems.size(); ++k) {
        if (!problems[k]) throw std::invalid_argument("ceres_shim: SolveBatch: problem " + std::to_string(k) + " is NULL");
        for (size_t q = 0; q < k; ++q)
            if (problems[q] == problems[k]) throw std::invalid_argument("ceres_shim: SolveBatch: problem " + std::to_string(k) + " is in the batch twice");
        if (problems[k]->image_blocks_.empty() || !problems[k]->obs_pose_.empty())
            throw std::invalid_argument("ceres_shim: SolveBatch: problem " + std::to_string(k) + " must hold ImageError blocks and nothing else");
    }
    if (options.trust_region_strategy_type == DOGLEG) throw std::invalid_argument("ceres_shim: SolveBatch: ImageError blocks are solved with Levenberg-Marquardt only");
    std::vector<ssba_problem *> hs;
    for (size_t k = 0; k < problems.size(); ++k) {
        int rc = 0;
        if (const char *where = shim_prepare(*problems[k], &rc))
            throw std::runtime_error(std::string("ceres_shim: SolveBatch: problem ") + std::to_string(k) + ": " + where + ": " + ssba_status_string(rc) + " (" + ssba_last_error() + ")");
        hs.push_back(problems[k]->h_);
    }
    const ssba_options o = shim_options(options);
    std::vector<ssba_summary> s(problems.size());
    std::vector<int> st(problems.size(), 0);
    const int rc = ssba_image_solve_batch(hs.data(), (uint32_t)hs.size(), &o, 0, s.data(), st.data());
    bool member = false;
    for (int x : st) member = member || x != 0;
    if (rc && !member) {
        const std::string msg = std::string("ssba_image_solve_batch: ") + ssba_status_string(rc) + " (" + ssba_last_error() + ")";
        if (rc == SSBA_ERR_INVALID_ARGUMENT || rc == SSBA_ERR_UNSUPPORTED || rc == SSBA_ERR_STATE) throw std::invalid_argument(msg);
        throw std::runtime_error(msg);
    }
    summaries->assign(problems.size(), Solver::Summary());
    for (size_t k = 0; k < problems.size(); ++k) {
        if (st[k] && st[k] != SSBA_ERR_NUMERICAL_FAILURE) {
            (*summaries)[k].termination_type = FAILURE;
            (*summaries)[k].message = std::string("ssba_image_solve_batch: ") + ssba_status_string(st[k]);
        } else shim_summary(s[k], &(*summaries)[k]);
    }
}

// ceres::Covariance (tests/dataset_vo_sun.cpp:159-183): Compute evaluates the requested blocks of (J^T J)^-1 in the
// tangent space at the problem's current parameter values (loss-corrected Jacobian, as Ceres' default
// apply_loss_function = true).  Pairs may be (pose | point, pose | point).  A request made only of diagonal pose blocks runs
// ssba_pose_covariance per pose (as it always has); any other request is one ssba_covariance_blocks call.
// GetCovarianceBlockInTangentSpace copies a computed pair out in either order (row-major, 6 x 6 / 6 x 3 / 3 x 6 / 3 x 3);
// GetCovarianceBlock does the same in ambient coordinates, which exist for points only (a pose's would be 12 x 12).
class Covariance {
 public:
    struct Options {
        int num_threads = 1;
        CovarianceAlgorithmType algorithm_type = SPARSE_QR;
        SparseLinearAlgebraLibraryType sparse_linear_algebra_library_type = SUITE_SPARSE;
        int null_space_rank = 0;
        bool apply_loss_function = true;
    };
    explicit Covariance(const Options &options) : options_(options) {}
    bool Compute(const std::vector<std::pair<const double *, const double *>> &blocks, Problem *problem) {
        Problem &P = *problem;
        blocks_.clear();
        message_.clear();
        if (!P.intensity_.empty() || !P.normals_.empty()) { message_ = "covariance is not available with lighting terms"; return false; }
        if (P.pose_blocks_.empty()) { message_ = "no pose blocks"; return false; }
        int rc = 0;
        const char *where = shim_prepare(P, &rc);      // the handle of the preceding Solve when nothing changed since
        bool diagonal_poses = true;
        std::vector<ssba_cov_block> req;
        for (size_t i = 0; !where && i < blocks.size(); ++i) {
            double *a = const_cast<double *>(blocks[i].first), *b = const_cast<double *>(blocks[i].second);
            ssba_cov_block r;
            if (!kind_index(P, a, &r.kind_a, &r.index_a) || !kind_index(P, b, &r.kind_b, &r.index_b)) {
                message_ = "a requested parameter block is not in the problem";
                rc = SSBA_ERR_INVALID_ARGUMENT;
                where = "Covariance::Compute";
                break;
            }
            diagonal_poses = diagonal_poses && a == b && r.kind_a == SSBA_COV_POSE;
            req.push_back(r);
        }
        if (!where && diagonal_poses) {
            for (size_t i = 0; !where && i < blocks.size(); ++i) {
                Block b(blocks[i].first, blocks[i].second, 6, 6);
                if ((rc = ssba_pose_covariance(P.h_, req[i].index_a, b.cov.data()))) where = "ssba_pose_covariance";
                else blocks_.push_back(b);
            }
        } else if (!where) {
            size_t total = 0;
            for (size_t i = 0; i < req.size(); ++i) total += dim(req[i].kind_a) * dim(req[i].kind_b);
            std::vector<double> out(total > 0 ? total : 1);
            if ((rc = ssba_covariance_blocks(P.h_, req.data(), req.size(), out.data()))) where = "ssba_covariance_blocks";
            for (size_t i = 0, o = 0; !where && i < req.size(); ++i) {
                Block b(blocks[i].first, blocks[i].second, dim(req[i].kind_a), dim(req[i].kind_b));
                std::copy(out.begin() + o, out.begin() + o + b.cov.size(), b.cov.begin());
                o += b.cov.size();
                blocks_.push_back(b);
            }
        }
        if (where && message_.empty()) message_ = std::string(where) + ": " + ssba_status_string(rc) + " (" + ssba_last_error() + ")";
        if (where) blocks_.clear();
        return where == nullptr;     // like Ceres: false on a rank-deficient Jacobian (no gauge constraint)
    }
    bool GetCovarianceBlockInTangentSpace(const double *a, const double *b, double *out) const {
        for (const Block &blk : blocks_) {
            if (blk.a == a && blk.b == b) { std::memcpy(out, blk.cov.data(), blk.cov.size() * sizeof(double)); return true; }
            if (blk.a == b && blk.b == a) {      // the transpose of a computed pair
                for (int r = 0; r < blk.rows; ++r)
                    for (int c = 0; c < blk.cols; ++c) out[(size_t)c * blk.rows + r] = blk.cov[(size_t)r * blk.cols + c];
                return true;
            }
        }
        return false;
    }
    // ambient coordinates: a point's are its tangent space; a pose's (12 x 12 over the stored 3x4 matrix) are refused
    bool GetCovarianceBlock(const double *a, const double *b, double *out) {
        for (const Block &blk : blocks_)
            if ((blk.a == a && blk.b == b) || (blk.a == b && blk.b == a)) {
                if (blk.rows != 3 || blk.cols != 3) {
                    message_ = "GetCovarianceBlock: the ambient covariance of a pose block (12 x 12) is not available; use "
                               "GetCovarianceBlockInTangentSpace";
                    return false;
                }
                return GetCovarianceBlockInTangentSpace(a, b, out);
            }
        return false;
    }
    const std::string &message() const { return message_; }

 private:
    struct Block {
        Block(const double *a_, const double *b_, int r, int c) : a(a_), b(b_), rows(r), cols(c), cov((size_t)r * c) {}
        const double *a, *b;
        int rows, cols;
        std::vector<double> cov;
    };
    static int dim(uint32_t kind) { return kind == SSBA_COV_POINT ? 3 : 6; }
    static bool kind_index(Problem &P, double *x, uint32_t *kind, uint32_t *index) {
        if (P.pose_index_.count(x)) { *kind = SSBA_COV_POSE; *index = P.pose_index_[x]; return true; }
        if (P.point_index_.count(x)) { *kind = SSBA_COV_POINT; *index = P.point_index_[x]; return true; }
        return false;
    }
    Options options_;
    std::vector<Block> blocks_;
    std::string message_;
};

}  // namespace ceres
#endif
