// sparse_stereo_sequence_gpu -- from raw stereo frames to a bundle-adjusted trajectory on the sparse path: feature tracks on the
// device (ceres_slam::FeatureTracker, include/ceres_slam_amd/feature_tracks.hpp), the VO initial guess on the device
// (DatasetProblem::compute_initial_guess = ssba_frontend_vo), then the solve of tests/dataset_vo.cpp:22-85 through the shim.
// It reads the raw file of examples/dense_stereo_sequence_gpu.cpp (its header states the layout; synth.write_stereo_sequence
// writes it): the frames, the camera and the matcher's parameters are used, the pyramid fields are not.
//
// usage: sparse_stereo_sequence_gpu sequence.raw [--sgbm] [--fast-threshold <n>] [--max-features <n>] [--min-track-length <n>]
//            [--temporal-radius <r>] [--subpixel] [--max-sad <s>] [--huber <a>] [--stream <W> [--odometry]]
// --sgbm takes the disparities from the semi-global matcher (StereoSGBM over all pairs in shared launches, sub-pixel) instead
// of from left-right feature matches (whole pixels).  --temporal-radius gates the frame-to-frame matches to r pixels.
// --subpixel refines every observation to 1/256 pixel against its track's first patch (FeatureTracker::subpixel), --max-sad
// drops refined observations whose patch difference exceeds s, and --huber puts a ceres::HuberLoss(a) on every residual block.
// --stream W pushes the frames one by one into a ceres_slam::FeatureTrackStream, as a camera would deliver them.  After every
// push from the second on it takes the window of the last min(W, pushed) frames, runs the front end and the solve on it from the
// trajectory's pose of the window's oldest frame (which stays constant), and the solved poses replace the trajectory's: the
// newest pose is chained on, the W - 1 before it are refined once more.  With W >= the number of frames and whole pixels the
// last window is the whole sequence and the output is that of the run without the flag.
// --odometry (with --stream W only) prints the trajectory from the stream's own poses instead: every push triangulates the matches
// to the frame before, runs the 3-point RANSAC and the two-view refinement on the device and chains the pose
// (FeatureTrackStream::enable_odometry / pose), so there is no window, no front end and no solve per frame; --huber is not used.
// Output (17 significant digits): one line "frame <k> <12 doubles of T_k_0>" per frame, frame 0 the identity.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <vector>

#include "ceres_slam_amd/ceres_shim.hpp"
#include "ceres_slam_amd/dataset_problem.hpp"
#include "ceres_slam_amd/feature_tracks.hpp"

// tests/dataset_vo.cpp:22-85 over all states, unit stiffness
static bool solveAll(ceres_slam::DatasetProblem &dataset, double huber) {
    ceres::Problem problem;
    ceres::LossFunction *loss = huber > 0.0 ? new ceres::HuberLoss(huber) : NULL;
    const double *var = dataset.stereo_obs_var.data();
    const double stiffness[9] = {1.0 / std::sqrt(var[0]), 0, 0, 0, 1.0 / std::sqrt(var[1]), 0, 0, 0, 1.0 / std::sqrt(var[2])};
    ceres::LocalParameterization *se3_perturbation = ceres_slam::SE3Perturbation::Create();
    for (ceres_slam::uint k = 0; k < dataset.num_states; ++k) {
        bool used = false;
        for (ceres_slam::uint i : dataset.obs_indices_at_state(k)) {
            const ceres_slam::uint j = dataset.point_ids[i];
            if (j >= dataset.num_points || !dataset.initialized_point[j]) continue;     // only initialised map points (:45)
            ceres::CostFunction *cost = ceres_slam::StereoReprojectionErrorAutomatic::Create(dataset.camera, dataset.stereo_obs_list[i].data(), stiffness);
            problem.AddResidualBlock(cost, loss, dataset.poses[k].data(), dataset.map_points[j].data());
            used = true;
        }
        if (used) problem.SetParameterization(dataset.poses[k].data(), se3_perturbation);
    }
    problem.SetParameterBlockConstant(dataset.poses[0].data());
    ceres::Solver::Options solver_options;
    solver_options.max_num_iterations = 1000;
    solver_options.use_nonmonotonic_steps = true;
    ceres::Solver::Summary summary;
    ceres::Solve(solver_options, &problem, &summary);
    std::cerr << summary.BriefReport() << std::endl;
    return summary.IsSolutionUsable();
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::cerr << "usage: sparse_stereo_sequence_gpu sequence.raw [--sgbm] [--fast-threshold <n>] [--max-features <n>] [--min-track-length <n>]"
                     " [--temporal-radius <r>] [--subpixel] [--max-sad <s>] [--huber <a>] [--stream <W> [--odometry]]" << std::endl;
        return EXIT_FAILURE;
    }
    ceres_slam::FeatureTracker tracker;
    bool use_sgbm = false;
    double huber = 0.0;
    int stream_window = 0;
    bool odometry = false;
    for (int a = 2; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--sgbm")) use_sgbm = true;
        else if (!std::strcmp(argv[a], "--fast-threshold") && a + 1 < argc) tracker.params.fast_threshold = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--max-features") && a + 1 < argc) tracker.params.max_features = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--min-track-length") && a + 1 < argc) tracker.params.min_track_length = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--temporal-radius") && a + 1 < argc) tracker.params.temporal_radius = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--subpixel")) tracker.subpixel = true;
        else if (!std::strcmp(argv[a], "--max-sad") && a + 1 < argc) tracker.refine.max_sad = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--huber") && a + 1 < argc) huber = std::atof(argv[++a]);
        else if (!std::strcmp(argv[a], "--stream") && a + 1 < argc) {
            stream_window = std::atoi(argv[++a]);
            if (stream_window < 1) { std::cerr << "--stream takes a window of at least 1 frame, not " << argv[a] << std::endl; return EXIT_FAILURE; }
        }
        else if (!std::strcmp(argv[a], "--odometry")) odometry = true;
        else { std::cerr << "unknown option " << argv[a] << std::endl; return EXIT_FAILURE; }
    }
    if (odometry && stream_window < 1) { std::cerr << "--odometry needs --stream <W>: the poses are the stream's own" << std::endl; return EXIT_FAILURE; }
    FILE *f = std::fopen(argv[1], "rb");
    int32_t head[8], sg[11];
    double scale_cam[6], start[12];
    if (!f || std::fread(head, sizeof head, 1, f) != 1 || std::fread(scale_cam, sizeof scale_cam, 1, f) != 1 || std::fread(start, sizeof start, 1, f) != 1 ||
        std::fread(sg, sizeof sg, 1, f) != 1 || head[0] < 2 || head[1] <= 0 || head[2] <= 0) {
        std::cerr << "cannot read " << argv[1] << std::endl;
        return EXIT_FAILURE;
    }
    const int frames = head[0], rows = head[1], cols = head[2];
    const size_t npix = (size_t)rows * cols;
    std::vector<uint8_t> left(npix * frames), right(npix * frames);
    for (int k = 0; k < frames; ++k)
        if (std::fread(&left[npix * k], 1, npix, f) != npix || std::fread(&right[npix * k], 1, npix, f) != npix) {
            std::cerr << "short file " << argv[1] << std::endl;
            return EXIT_FAILURE;
        }
    std::fclose(f);
    ceres_slam::DatasetProblem::CameraPtr camera = std::make_shared<const ceres_slam::StereoCamera>(scale_cam[1], scale_cam[2], scale_cam[3], scale_cam[4], scale_cam[5]);

    std::vector<ceres_slam::SE3> trajectory(frames);
    bool usable = true;
    try {
        std::vector<int16_t> disp16;
        if (use_sgbm) {
            ceres_slam::StereoSGBM sgbm(sg[0], sg[1], sg[2], sg[3], sg[4], sg[5], sg[6], sg[7], sg[8], sg[9], sg[10] != 0);
            std::vector<ceres_slam::Image8> l, r;
            for (int k = 0; k < frames; ++k) {
                l.push_back(ceres_slam::Image8(rows, cols, &left[npix * k]));
                r.push_back(ceres_slam::Image8(rows, cols, &right[npix * k]));
            }
            std::vector<ceres_slam::DisparityMap> maps;
            sgbm(l, r, maps);
            disp16.resize(npix * frames);
            for (int k = 0; k < frames; ++k) std::memcpy(&disp16[npix * k], maps[k].disp16.data(), npix * sizeof(int16_t));
        }
        if (stream_window > 0) {
            ceres_slam::FeatureTrackStream stream(rows, cols, stream_window, tracker.params, tracker.subpixel ? &tracker.refine : nullptr);
            if (odometry) stream.enable_odometry(*camera);
            for (int k = 0; k < frames; ++k) {
                const uint32_t kept = stream.push(&left[npix * k], use_sgbm ? nullptr : &right[npix * k], use_sgbm ? &disp16[npix * k] : nullptr);
                std::cerr << "frame " << k << ": " << kept << " observations, " << stream.num_dropped << " dropped by the refinement" << std::endl;
                if (odometry) {
                    ssba_track_pose_info info;
                    trajectory[k] = stream.pose(nullptr, &info);
                    std::cerr << "frame " << k << ": status " << info.status << ", " << info.num_inliers << " inliers of " << info.num_matches << " matches, "
                              << info.num_iterations << " iteration records, cost " << info.initial_cost << " -> " << info.final_cost << std::endl;
                    continue;
                }
                if (!k) continue;
                const int w = std::min(stream_window, k + 1), oldest = k + 1 - w;
                ceres_slam::DatasetProblem window;
                stream.window(w, camera, &window, trajectory[oldest]);
                std::cerr << window.stereo_obs_list.size() << " observations of " << window.num_points << " tracks in frames " << oldest << " ... " << k << std::endl;
                if (!window.compute_initial_guess()) return EXIT_FAILURE;
                usable = solveAll(window, huber) && usable;       // an earlier window's poses seed the later ones
                for (int i = 0; i < w; ++i) trajectory[oldest + i] = window.poses[i];
            }
        } else {
            ceres_slam::DatasetProblem dataset;
            tracker.track(left.data(), use_sgbm ? nullptr : right.data(), use_sgbm ? disp16.data() : nullptr, frames, rows, cols, camera, &dataset);
            std::cerr << dataset.stereo_obs_list.size() << " observations of " << dataset.num_points << " tracks in " << frames << " frames" << std::endl;
            if (tracker.subpixel) std::cerr << tracker.num_dropped << " observations dropped by the refinement" << std::endl;
            if (!dataset.compute_initial_guess()) return EXIT_FAILURE;
            usable = solveAll(dataset, huber);
            trajectory = dataset.poses;
        }
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return EXIT_FAILURE;
    }

    std::cout.precision(17);
    for (int k = 0; k < frames; ++k) {
        std::cout << "frame " << k;
        for (int c = 0; c < 12; ++c) std::cout << " " << trajectory[k].data()[c];
        std::cout << std::endl;
    }
    return usable ? EXIT_SUCCESS : EXIT_FAILURE;
}
