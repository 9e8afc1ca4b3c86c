// CPU-only check of the rule that keeps relative-pose blocks between neighbouring free poses on the windowed layout
// (ceres_slam_amd/csrc/ssba_layout.cpp), built by tests/test_host_odometry_layout.py with -fsanitize=address,undefined and once
// with -fsanitize=thread.  Case A: a chain of blocks (k, k + 1) over 27 free poses stays windowed, block (f, f + 1) exists for
// every f (the super-block boundaries 11|12 and 23|24 included, also when no landmark crosses 11|12), and every block's list holds
// exactly the relative-pose blocks added for its pair, in the order they were added, with the transpose flag of a block added as
// (k + 1, k).  Case B: a loop block, a block over two free indices, a problem without observations stay on the general layout.
// Case C: a constant pose between two free ones makes them neighbours; a chain through a constant pose couples nothing across it.
// Exit code 0 = all invariants hold.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ssba.h"
#include "ssba_layout.h"
#include "ssba_types.h"

using namespace ssba;

struct Prob {
    uint32_t P = 0, L = 0;
    std::vector<uint32_t> obs_pose, obs_point;
    std::vector<double> obs_uvd;
    std::vector<uint8_t> pose_const;
    std::vector<PoseFactor> pfs;
    std::vector<RelFactor> rfs;
};

// landmark j is seen by `track` consecutive poses starting where j sits along the trajectory; cut >= 0 leaves out every
// landmark seen on both sides of cut | cut + 1
static Prob make(uint32_t P, uint32_t L, uint32_t track, int cut = -1) {
    Prob q;
    q.P = P;
    q.pose_const.assign(P, 0);
    for (uint32_t j = 0; j < L; ++j) {
        const uint32_t first = (uint32_t)((uint64_t)j * (P - track + 1) / L);
        if (cut >= 0 && (int)first <= cut && (int)(first + track - 1) > cut) continue;
        for (uint32_t k = first; k < first + track; ++k) {
            q.obs_pose.push_back(k); q.obs_point.push_back(q.L);
            q.obs_uvd.push_back(1.0 + k); q.obs_uvd.push_back(2.0 + j); q.obs_uvd.push_back(3.0);
        }
        ++q.L;
    }
    return q;
}
static void add_rel(Prob &q, uint32_t a, uint32_t b, double tag) {
    RelFactor f{};
    f.pose1 = a; f.pose2 = b;
    f.T_ref[0] = tag;       // recognised again in the half entries
    for (int i = 0; i < 3; ++i) f.T_ref[3 + 4 * i] = 1.0;
    for (int i = 0; i < 6; ++i) f.S[7 * i] = 1.0;
    q.rfs.push_back(f);
}
static void add_prior(Prob &q, uint32_t k) {
    PoseFactor f{};
    f.pose = k; f.type = 0;
    for (int i = 0; i < 3; ++i) f.data[3 + 4 * i] = 1.0;
    for (int i = 0; i < 6; ++i) f.S[7 * i] = 1.0;
    q.pfs.push_back(f);
}

static int fail(const char *name, const std::string &what) { printf("FAIL (%s): %s\n", name, what.c_str()); return 1; }

static int build(const char *name, const Prob &q, Layout &lay) {
    const std::vector<double> none;
    const std::vector<uint32_t> nomat;
    LayoutInput in{q.P, q.L, q.obs_pose, q.obs_point, q.obs_uvd, q.pose_const, false, none, false, 0, nomat,
                   none, none, false, q.pfs, q.rfs, 1, false, false, false};
    std::string err;
    const int rc = build_layout(in, lay, err);
    if (rc != SSBA_OK) return fail(name, "rejected: " + err);
    return 0;
}

// device order of the half entries: sorted by pose, the order they were added kept inside a pose (ssba_finalize)
static std::vector<uint32_t> device_positions(const Layout &lay, uint32_t P) {
    std::vector<uint32_t> at(P + 1, 0), pos(lay.pfs.size());
    for (auto &f : lay.pfs) at[f.pose + 1]++;
    for (uint32_t k = 0; k < P; ++k) at[k + 1] += at[k];
    for (size_t i = 0; i < lay.pfs.size(); ++i) pos[i] = at[lay.pfs[i].pose]++;
    return pos;
}

// the windowed layout with a block (f, f + 1) for exactly the pairs in `pairs` beyond those the landmarks give, and lists
// that hold exactly the caller's relative-pose blocks between two free poses
static int check_windowed(const char *name, const Prob &q, const std::vector<std::pair<int, int>> &no_block = {}) {
    Layout lay;
    if (build(name, q, lay)) return 1;
    if (lay.dense || lay.wide_sys || lay.nborder) return fail(name, "not on the windowed layout");
    if (lay.sblk_a.size() != lay.n_sblk || lay.sblk_start.size() != (size_t)lay.n_sblk + 1) return fail(name, "block list sizes");
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> blk_of;
    for (uint32_t b = 0; b < lay.n_sblk; ++b) {
        if (lay.sblk_b[b] < lay.sblk_a[b] || lay.sblk_b[b] - lay.sblk_a[b] > (uint32_t)SBP || lay.sblk_b[b] >= (uint32_t)lay.nfree) return fail(name, "block outside the envelope");
        if (b && !(std::make_pair(lay.sblk_a[b - 1], lay.sblk_b[b - 1]) < std::make_pair(lay.sblk_a[b], lay.sblk_b[b]))) return fail(name, "blocks not in (a, b) order");
        blk_of[{lay.sblk_a[b], lay.sblk_b[b]}] = b;
    }
    for (int f = 0; f < lay.nfree; ++f) if (!blk_of.count({(uint32_t)f, (uint32_t)f})) return fail(name, "a free pose without its diagonal block");
    // what the caller added, per pair of free indices, in order: (tag, transposed)
    std::map<std::pair<uint32_t, uint32_t>, std::vector<std::pair<double, bool>>> want;
    for (auto &rf : q.rfs) {
        const int f1 = lay.pose_free[rf.pose1], f2 = lay.pose_free[rf.pose2];
        if (f1 < 0 || f2 < 0) continue;
        if (f1 - f2 != 1 && f2 - f1 != 1) return fail(name, "a block over more than one free index on the windowed layout");
        want[{(uint32_t)std::min(f1, f2), (uint32_t)std::max(f1, f2)}].push_back({rf.T_ref[0], f1 > f2});
    }
    if (want.empty()) {
        if (!lay.sblk_rf_start.empty() || !lay.sblk_rf.empty()) return fail(name, "relative-pose lists without a coupled pair");
    } else {
        if (lay.sblk_rf_start.size() != (size_t)lay.n_sblk + 1 || lay.sblk_rf_start[0] != 0 || lay.sblk_rf_start.back() != lay.sblk_rf.size())
            return fail(name, "relative-pose list offsets");
        if (lay.bandwidth < 1) return fail(name, "bandwidth 0 with a coupled pair");
    }
    const std::vector<uint32_t> pos = device_positions(lay, q.P);
    std::vector<int> host_of(lay.pfs.size(), -1);
    for (size_t i = 0; i < pos.size(); ++i) host_of[pos[i]] = (int)i;
    size_t listed = 0;
    for (auto &w : want) {
        if (!blk_of.count(w.first)) return fail(name, "no block (" + std::to_string(w.first.first) + ", " + std::to_string(w.first.second) + ") for a relative-pose block");
        const uint32_t b = blk_of[w.first];
        const uint32_t r0 = lay.sblk_rf_start[b], r1 = lay.sblk_rf_start[b + 1];
        if (r1 < r0 || r1 - r0 != w.second.size()) return fail(name, "list length of block (" + std::to_string(w.first.first) + ", " + std::to_string(w.first.second) + ")");
        for (uint32_t x = r0; x < r1; ++x) {
            const uint32_t ent = lay.sblk_rf[x], e = ent & 0x7FFFFFFFu;
            if (e >= lay.pfs.size()) return fail(name, "list entry out of range");
            const PoseFactor &h = lay.pfs[host_of[e]];
            if (h.type != 2 || h.data[13] != 1.0 || h.data[14] < 0.0) return fail(name, "list entry is not the first half of a block between free poses");
            if (h.data[0] != w.second[x - r0].first) return fail(name, "blocks of a pair not in the order they were added");
            if (((ent >> 31) != 0) != w.second[x - r0].second) return fail(name, "transpose flag");
            const uint32_t fa = (uint32_t)lay.pose_free[h.pose], fb = (uint32_t)lay.pose_free[(uint32_t)h.data[12]];
            if (std::min(fa, fb) != w.first.first || std::max(fa, fb) != w.first.second) return fail(name, "list entry of another pair");
            const PoseFactor &h2 = lay.pfs[(size_t)h.data[14]];      // (host index in Layout::pfs)
            if (h2.type != 3 || h2.pose != (uint32_t)h.data[12] || (uint32_t)h2.data[12] != h.pose) return fail(name, "second half");
        }
        listed += r1 - r0;
    }
    if (!want.empty() && listed != lay.sblk_rf.size()) return fail(name, "list entries on blocks without a relative-pose block");
    for (auto &nb : no_block)
        if (blk_of.count({(uint32_t)nb.first, (uint32_t)nb.second})) return fail(name, "a block that nothing contributes to");
    printf("ok   %-46s %3d free  %4u blocks  %3zu relative-pose entries\n", name, lay.nfree, lay.n_sblk, lay.sblk_rf.size());
    return 0;
}

static int check_dense(const char *name, const Prob &q) {
    Layout lay;
    if (build(name, q, lay)) return 1;
    if (!lay.dense || lay.wide_sys) return fail(name, "not on the general layout");
    if (!lay.sblk_rf_start.empty() || !lay.sblk_rf.empty()) return fail(name, "windowed relative-pose lists on the general layout");
    printf("ok   %-46s general layout\n", name);
    return 0;
}

int main() {
    int bad = 0;
    const uint32_t P = 27, L = 810, track = 4;
    auto chain = [&](Prob &q) { for (uint32_t k = 0; k + 1 < q.P; ++k) add_rel(q, k, k + 1, 100.0 + k); };
    // ---- A: a chain on the windowed layout
    {
        Prob q = make(P, L, track);
        add_prior(q, 0);
        chain(q);
        bad += check_windowed("A chain", q);
        Prob c = make(P, L, track, 11);
        add_prior(c, 0);
        chain(c);
        bad += check_windowed("A chain, no landmark across 11|12", c);
        Prob m = make(P, L, track, 11);      // several blocks on one pair, one of them added as (k + 1, k); a prior between the halves
        add_rel(m, 11, 12, 1.0); add_prior(m, 12); add_rel(m, 12, 11, 2.0); add_rel(m, 11, 12, 3.0);
        add_rel(m, 24, 23, 4.0); add_rel(m, 1, 0, 5.0);
        bad += check_windowed("A repeated and reversed blocks", m);
        Prob n = make(P, L, track, 11);      // without blocks nothing couples 11 and 12
        bad += check_windowed("A no blocks, no landmark across 11|12", n, {{11, 12}});
    }
    // ---- B: problems that stay on the general layout
    {
        Prob q = make(P, L, track);
        add_prior(q, 0);
        chain(q);
        Prob loop = q;
        add_rel(loop, 0, 26, 7.0);
        bad += check_dense("B chain + loop block (0, 26)", loop);
        Prob skip = q;
        add_rel(skip, 3, 5, 8.0);
        bad += check_dense("B chain + block (3, 5), pose 4 free", skip);
        Prob graph = q;
        graph.L = 0; graph.obs_pose.clear(); graph.obs_point.clear(); graph.obs_uvd.clear();
        bad += check_dense("B pose graph without observations", graph);
    }
    // ---- C: pairs made consecutive by a constant pose
    {
        Prob q = make(P, L, track);
        add_prior(q, 0);
        chain(q);
        add_rel(q, 3, 5, 8.0);
        q.pose_const[4] = 1;
        bad += check_windowed("C block (3, 5) over constant pose 4", q);
        Prob c = make(P, L, track, 11);
        add_prior(c, 0);
        chain(c);
        c.pose_const[12] = 1;       // blocks (11, 12) and (12, 13) become unary halves: free indices 11 and 12 (pose 13) stay uncoupled
        bad += check_windowed("C chain through constant pose 12", c, {{11, 12}});
    }
    if (bad) { printf("%d case(s) failed\n", bad); return 1; }
    printf("all invariants hold\n");
    return 0;
}
