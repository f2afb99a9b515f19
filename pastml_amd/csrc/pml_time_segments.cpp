// The segment plan of pml_history_through_time (pml_time_segments.h).  Plain C++, no HIP.
#include "pml_time_segments.h"

#include <algorithm>
#include <cmath>

namespace {

struct Segment {
    int node, starts;
    double s1, w, r, u;
};

// calls emit(bin, segment) for every segment of the branch above n, bins ascending; the pseudo-bin M last
template <class Emit>
void branch_segments(int n, double tp, double tn, const double* T, int M, Emit emit) {
    const double h = tn - tp;
    if (h == 0.0) {
        if (tn < T[0] || tn > T[M]) return;
        const int m = tn == T[M] ? M - 1 : (int)(std::upper_bound(T, T + M + 1, tn) - T) - 1;
        emit(m, Segment{n, 0, 0.0, 1.0, 0.0, 1.0});
        return;
    }
    int m = std::max(0, (int)(std::upper_bound(T, T + M + 1, tp) - T) - 1);
    for (; m < M && T[m] < tn; ++m) {
        const double lo = std::max(T[m], tp), hi = std::min(T[m + 1], tn);
        if (!(hi > lo)) continue;
        emit(m, Segment{n, tp <= T[m] ? 1 : 0, (lo - tp) / h, (hi - lo) / h, (tn - hi) / h, (tn - lo) / h});
    }
    if (tp <= T[M] && T[M] < tn) emit(M, Segment{n, 1, (T[M] - tp) / h, 0.0, (tn - T[M]) / h, (tn - T[M]) / h});
}

}   // namespace

std::string pml_plan_time_segments(const int* parent, const double* node_time, int N, const double* boundaries, int M,
                                   PmlTimeSegments& out) {
    if (M < 1) return "M = " + std::to_string(M) + ": at least one time bin (two boundaries) is needed";
    if (N < 1 || !parent || !node_time || !boundaries) return "no nodes, or an array is missing";
    for (int m = 0; m <= M; ++m)
        if (!std::isfinite(boundaries[m])) return "boundary " + std::to_string(m) + " is not finite";
    for (int m = 0; m < M; ++m)
        if (!(boundaries[m] < boundaries[m + 1]))
            return "boundary " + std::to_string(m + 1) + " is not above boundary " + std::to_string(m) +
                   ": the boundaries must be strictly ascending";
    for (int n = 0; n < N; ++n) {
        if (!std::isfinite(node_time[n])) return "the time of node " + std::to_string(n) + " is not finite";
        if (parent[n] >= N || parent[n] == n) return "the parent of node " + std::to_string(n) + " is no node";
    }
    for (int n = 0; n < N; ++n)
        if (parent[n] >= 0 && node_time[n] < node_time[parent[n]])
            return "node " + std::to_string(n) + " is earlier than its parent " + std::to_string(parent[n]);
    // two walks over the nodes in ascending order: the bins' sizes, then the segments into their places (ids ascend in a bin)
    std::vector<int> off(M + 2, 0);
    for (int n = 0; n < N; ++n)
        if (parent[n] >= 0)
            branch_segments(n, node_time[parent[n]], node_time[n], boundaries, M, [&](int m, const Segment&) { ++off[m + 1]; });
    for (int m = 0; m <= M; ++m) off[m + 1] += off[m];
    PmlTimeSegments plan;
    plan.M = M;
    plan.bin_off = off;
    const size_t total = (size_t)off[M + 1];
    plan.node.resize(total);
    plan.starts.resize(total);
    plan.frac.resize(4 * total);
    std::vector<int> at(off.begin(), off.end() - 1);
    for (int n = 0; n < N; ++n)
        if (parent[n] >= 0)
            branch_segments(n, node_time[parent[n]], node_time[n], boundaries, M, [&](int m, const Segment& s) {
                const size_t i = (size_t)at[m]++;
                plan.node[i] = s.node;
                plan.starts[i] = s.starts;
                plan.frac[4 * i] = s.s1;
                plan.frac[4 * i + 1] = s.w;
                plan.frac[4 * i + 2] = s.r;
                plan.frac[4 * i + 3] = s.u;
            });
    out = std::move(plan);
    return "";
}

PmlTimePieces pml_cut_time_pieces(const PmlTimeSegments& plan, int piece, bool with_points) {
    PmlTimePieces out;
    const int bins = plan.M + (with_points ? 1 : 0);
    out.bin_piece_off.assign(1, 0);
    out.piece_off.assign(1, 0);
    for (int m = 0; m < bins; ++m) {
        for (int i = plan.bin_off[m]; i < plan.bin_off[m + 1]; i += piece) out.piece_off.push_back(std::min(i + piece, plan.bin_off[m + 1]));
        out.bin_piece_off.push_back(out.n_pieces());
    }
    return out;
}

PmlTimeSegmentEnds pml_time_segment_ends(const PmlTimeSegments& plan) {
    PmlTimeSegmentEnds out;
    const size_t total = (size_t)plan.n_segments();
    out.s2.assign(total, 1.0);
    out.ends.assign(total, 1);
    for (int m = 0; m < plan.M; ++m) {
        // the ids ascend within a bin: the branch's segment of the next bin by bisection
        const int* next = plan.node.data() + plan.bin_off[m + 1];
        const int* next_end = plan.node.data() + plan.bin_off[m + 2];
        for (int i = plan.bin_off[m]; i < plan.bin_off[m + 1]; ++i) {
            const int* at = std::lower_bound(next, next_end, plan.node[i]);
            if (at == next_end || *at != plan.node[i]) continue;
            out.s2[i] = plan.frac[4 * (size_t)(at - plan.node.data())];
            out.ends[i] = 0;
        }
    }
    return out;
}
