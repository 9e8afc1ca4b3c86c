// FeatureTracker -- from a stack of rectified stereo frames to a DatasetProblem (dataset_problem.hpp), on the device.
//
// The reference's stereo-odometry node (ros/src/ceres_slam/src/sparse_stereo_odometry_node.cpp:127-216) detects and describes
// features, matches left to right and frame to frame, and hands (u, v, d) rows with landmark ids to the back end.
// libssba_tracks.so (include/ssba_tracks.h) does that from raw 8-bit frames; this class puts its output where the drivers expect
// it: state_ids / point_ids / stereo_obs_list of a DatasetProblem, ready for compute_initial_guess and a solve through the shim.
// Link with -lssba_tracks -lssba.
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "ceres_slam_amd/dataset_problem.hpp"
#include "ssba_tracks.h"

namespace ceres_slam {

class FeatureTracker {
 public:
    //! ssba_track_default_params; set fields before track()
    ssba_track_params params;
    int device;
    //! observations refined to 1/256 pixel against each track's first patch (ssba_track_sequence_subpixel) under `refine`
    bool subpixel = false;
    //! ssba_track_default_refine_params; used when `subpixel` is set
    ssba_track_refine_params refine;
    //! after a track() with `subpixel`: the observations whose refinement failed and that were left out
    mutable uint64_t num_dropped = 0;

    explicit FeatureTracker(int device_ = -1) : device(device_) {
        ssba_track_default_params(&params);
        ssba_track_default_refine_params(&refine);
    }

    //! `frames` images of rows x cols in `left`, then exactly one of `right` (as many images) and `disp16` (as many int16 maps in
    //! the format StereoSGBM writes).  Fills `out`: the camera, one state per frame (the first pose is `first_pose`, the others
    //! start at the identity until compute_initial_guess runs), one uninitialised map point per track, the observations grouped
    //! by state in keypoint order, unit observation variances.  Throws std::runtime_error with the library's message on a refusal.
    void track(const uint8_t *left, const uint8_t *right, const int16_t *disp16, uint32_t frames, uint32_t rows, uint32_t cols,
               DatasetProblem::CameraPtr camera, DatasetProblem *out, const SE3 &first_pose = SE3()) const {
        if (!out) throw std::invalid_argument("FeatureTracker: NULL dataset");
        const uint64_t capacity = (uint64_t)frames * (uint64_t)(params.max_features > 0 ? params.max_features : 0);
        std::vector<uint32_t> state_start((size_t)frames + 1, 0), point_id(capacity ? capacity : 1);
        std::vector<double> uvd(3 * (capacity ? capacity : 1));
        uint64_t num_observations = 0;
        uint32_t num_points = 0;
        num_dropped = 0;
        const int rc = subpixel ? ssba_track_sequence_subpixel(left, right, disp16, frames, rows, cols, &params, device, capacity, state_start.data(),
                                                               point_id.data(), uvd.data(), &num_observations, &num_points, &refine, &num_dropped)
                                : ssba_track_sequence(left, right, disp16, frames, rows, cols, &params, device, capacity, state_start.data(), point_id.data(),
                                                      uvd.data(), &num_observations, &num_points);
        if (rc) throw std::runtime_error(std::string(ssba_status_string(rc)) + ": " + ssba_track_last_error());
        out->camera = camera;
        out->num_states = frames;
        out->num_points = num_points;
        out->poses.assign(frames, SE3());
        if (frames) out->poses[0] = first_pose;
        out->map_points.assign(num_points, Point());
        out->initialized_point.assign(num_points, false);
        for (int c = 0; c < 3; ++c) out->stereo_obs_var.v[c] = 1.0;
        out->state_ids.clear(); out->point_ids.clear(); out->stereo_obs_list.clear();
        for (uint32_t k = 0; k < frames; ++k)
            for (uint32_t i = state_start[k]; i < state_start[k + 1]; ++i) {
                out->state_ids.push_back(k);
                out->point_ids.push_back(point_id[i]);
                out->stereo_obs_list.push_back(DatasetProblem::Observation{{uvd[3 * (size_t)i], uvd[3 * (size_t)i + 1], uvd[3 * (size_t)i + 2]}});
            }
        out->rebuild_indices();
    }
};

}  // namespace ceres_slam
