// dense_stereo_sequence_gpu -- dense photometric alignment over a sequence of stereo frames, written against
// include/ceres_slam_amd/ceres_shim.hpp.  F frames give F - 1 pairs (left_k, right_k, left_{k+1}) that do not depend on each other:
// one image pyramid per pair (the matcher runs on left_k / right_k on the device), all of them aligned coarse to fine in ONE batched
// call (the batched ceres::SolveCoarseToFine: one shared solve per level), the relative poses composed into a trajectory.
//
//     int32  frames (>= 3), rows, cols, levels, disparity_level, interpolation (0 nearest, 1 bilinear), disparities_constant (0 | 1),
//            gradient_source (0 reference image, 1 tracked image)
//     double gradient_scale, fu, fv, cu, cv, b          the camera of level 0
//     double T_start[12]                                the start of every pair, [t | R row-major]
//     int32  min_disparity, num_disparities, block_size, p1, p2, disp12_max_diff, pre_filter_cap, uniqueness_ratio,
//            speckle_window_size, speckle_range, full_dp     the matcher's parameters (ssba_sgbm_params)
//     uint8  left_0, right_0, left_1, right_1, ...      rows * cols each, row-major
//
// usage: dense_stereo_sequence_gpu sequence.raw [--sequential] [--sequence] [--max-iterations <n>] [--huber <a>]
// --sequence builds ONE ceres_slam::ImageSequence from the frames instead of F - 1 pyramids: every frame is uploaded and prepared
// once and the matcher runs over all pairs in shared launches; the pyramids of the pairs are borrowed from it.  Same printed bytes.
// --sequential aligns the same pairs one by one (ceres::SolveCoarseToFine per pyramid); the printed poses are identical.
// --huber a puts ceres::HuberLoss(a) on the blocks of every level of every pyramid (ImagePyramid::SetHuberLoss).
// Output (17 significant digits): one line "frame <k> <12 doubles of T_k_0>" per frame, frame 0 the identity.
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
        std::cerr << "usage: dense_stereo_sequence_gpu sequence.raw [--sequential] [--sequence] [--max-iterations <n>] [--huber <a>]" << std::endl;
        return EXIT_FAILURE;
    }
    bool sequential = false, sequence = false;
    int max_iterations = -1;
    double huber_a = 0.0;
    for (int a = 2; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--sequential")) sequential = true;
        else if (!std::strcmp(argv[a], "--sequence")) sequence = true;
        else if (!std::strcmp(argv[a], "--max-iterations") && a + 1 < argc) max_iterations = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--huber") && a + 1 < argc) huber_a = std::atof(argv[++a]);
        else { std::cerr << "unknown option " << argv[a] << std::endl; return EXIT_FAILURE; }
    }
    FILE *f = std::fopen(argv[1], "rb");
    int32_t head[8], sg[11];
    double scale_cam[6], start[12];
    if (!f || std::fread(head, sizeof head, 1, f) != 1 || std::fread(scale_cam, sizeof scale_cam, 1, f) != 1 || std::fread(start, sizeof start, 1, f) != 1 ||
        std::fread(sg, sizeof sg, 1, f) != 1 || head[0] < 3 || head[1] <= 0 || head[2] <= 0 || head[3] <= 0 || head[3] > 31 || head[4] < 0 || head[4] >= head[3]) {
        std::cerr << "cannot read " << argv[1] << std::endl;
        return EXIT_FAILURE;
    }
    const int frames = head[0], rows = head[1], cols = head[2], levels = head[3], disparity_level = head[4], interpolation = head[5];
    const bool disparities_constant = head[6] != 0;
    const size_t npix = (size_t)rows * cols;
    std::vector<std::vector<uint8_t>> left((size_t)frames, std::vector<uint8_t>(npix)), right((size_t)frames, std::vector<uint8_t>(npix));
    for (int k = 0; k < frames; ++k)
        if (std::fread(left[k].data(), 1, npix, f) != npix || std::fread(right[k].data(), 1, npix, f) != npix) {
            std::cerr << "short file " << argv[1] << std::endl;
            return EXIT_FAILURE;
        }
    std::fclose(f);
    const ceres_slam::StereoCamera camera0(scale_cam[1], scale_cam[2], scale_cam[3], scale_cam[4], scale_cam[5]);
    ceres_slam::StereoSGBM sgbm(sg[0], sg[1], sg[2], sg[3], sg[4], sg[5], sg[6], sg[7], sg[8], sg[9], sg[10] != 0);

    const int pairs = frames - 1, coarsest = levels - 1;
    std::vector<std::unique_ptr<ceres_slam::ImagePyramid>> pyramids;
    std::unique_ptr<ceres_slam::ImageSequence> frames_once;
    std::vector<ceres_slam::ImagePyramid *> pyramid_ptrs;
    std::vector<double *> maps;
    std::vector<double> poses((size_t)pairs * 12);
    if (sequence) {
        std::vector<const uint8_t *> lp, rp;
        for (int k = 0; k < frames; ++k) { lp.push_back(left[k].data()); rp.push_back(right[k].data()); }
        frames_once.reset(new ceres_slam::ImageSequence(lp, rp, rows, cols, levels, disparity_level, sgbm, head[7], scale_cam[0]));
    }
    for (int k = 0; k < pairs; ++k) {
        if (sequence) {
            pyramid_ptrs.push_back(&frames_once->pyramid(k));
        } else {
            pyramids.emplace_back(new ceres_slam::ImagePyramid(left[k].data(), right[k].data(), left[k + 1].data(), rows, cols, levels, disparity_level, sgbm,
                                                               head[7], scale_cam[0]));
            pyramid_ptrs.push_back(pyramids.back().get());
        }
        if (huber_a > 0.0) pyramid_ptrs.back()->SetHuberLoss(huber_a);
        maps.push_back(pyramid_ptrs.back()->disparity(disparity_level).data());      // the blocks' memory: the matcher's map, downloaded once
        std::memcpy(&poses[(size_t)k * 12], start, sizeof start);
    }
    ceres::Solver::Options solver_options;
    solver_options.use_nonmonotonic_steps = true;
    if (max_iterations >= 0) solver_options.max_num_iterations = max_iterations;
    bool usable = true;
    if (sequential) {
        for (int k = 0; k < pairs; ++k) {
            std::vector<ceres::Solver::Summary> summaries;
            ceres::SolveCoarseToFine(solver_options, *pyramid_ptrs[k], camera0, &poses[(size_t)k * 12], maps[k], coarsest, interpolation, disparities_constant,
                                     &summaries);
            usable = usable && !summaries.empty() && summaries.back().IsSolutionUsable();
        }
    } else {
        std::vector<std::vector<ceres::Solver::Summary>> summaries;
        ceres::SolveCoarseToFine(solver_options, pyramid_ptrs, camera0, poses.data(), maps, coarsest, interpolation, disparities_constant, &summaries);
        for (const std::vector<ceres::Solver::Summary> &s : summaries) usable = usable && !s.empty() && s.back().IsSolutionUsable();
    }

    // T_{k+1,0} = T_{k+1,k} T_{k,0}
    double T[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::cout.precision(17);
    for (int k = 0; k < frames; ++k) {
        std::cout << "frame " << k;
        for (int c = 0; c < 12; ++c) std::cout << " " << T[c];
        std::cout << std::endl;
        if (k == pairs) break;
        const double *S = &poses[(size_t)k * 12];
        double N[12];
        for (int i = 0; i < 3; ++i) {
            N[i] = S[3 + 3 * i] * T[0] + S[4 + 3 * i] * T[1] + S[5 + 3 * i] * T[2] + S[i];
            for (int j = 0; j < 3; ++j) N[3 + 3 * i + j] = S[3 + 3 * i] * T[3 + j] + S[4 + 3 * i] * T[6 + j] + S[5 + 3 * i] * T[9 + j];
        }
        std::memcpy(T, N, sizeof T);
    }
    return usable ? EXIT_SUCCESS : EXIT_FAILURE;
}
