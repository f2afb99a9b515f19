// The segment plan of pml_history_through_time, made on the host: the branches of a dated forest cut at the boundaries
// T_0 < ... < T_M of M time bins (bin m = [T_m, T_{m+1}); the last one also contains T_M).
//
// A non-root node n with parent p and extent h = time_n - time_p > 0 has, in every bin with lo = max(T_m, time_p) <
// hi = min(T_{m+1}, time_n), one segment with the three fractions
//     s1 = (lo - time_p) / h,   w = (hi - lo) / h,   r = (time_n - hi) / h
// each ONE quotient of ONE difference of the given doubles -- never s2 - s1: a sliver of 1e-12 of a branch next to a node keeps
// all its digits -- and u = (time_n - lo) / h, the "1 - s1" of the lineage count, formed the same way.  A segment whose branch
// is alive at the bin's own boundary (time_p <= T_m < time_n, so lo == T_m) carries the flag `starts`: the lineages at T_m are
// summed over exactly those.  A branch with h == 0 has smoothed length only: one segment s1 = 0, w = 1, r = 0 (u = 1, no flag)
// in the bin that contains time_n, none if no bin does.  What lies outside [T_0, T_M] gives no segment.  The branches alive at
// the last boundary T_M (time_p <= T_M < time_n) are zero-width point segments (w = 0, flag set) of the pseudo-bin M.
//
// The segments are sorted by (bin, caller's node id); bin_off [M + 2] are the offsets of the bins 0 .. M - 1 and of the
// pseudo-bin M.  The plan depends on the tree, the times and the boundaries only -- not on a column.
// Plain C++ like pml_columns.h: built, tested and sanitised on any host (tests/time_segments_driver.cpp).
#pragma once
#include <string>
#include <vector>

#include "pml_schedule.h"   // (PML_PLAN)

struct PmlTimeSegments {
    int M = 0;
    std::vector<int> node;       // caller's id of the node below the branch
    std::vector<int> starts;     // 1: the branch is alive at the boundary its bin begins with
    std::vector<double> frac;    // [segments][4]: s1, w, r, u
    std::vector<int> bin_off;    // [M + 2]
    int n_segments() const { return (int)node.size(); }
    int n_interval_segments() const { return bin_off.empty() ? 0 : bin_off[M]; }   // (those of the bins proper)
};

// "" and the plan in `out`, or the reason -- which names the node or the index -- with `out` untouched: a child earlier than its
// parent, boundaries that are not strictly ascending, M < 1, a value that is not finite, a parent that is no node.
// parent [N]: -1 for a root; node_time [N]; boundaries [M + 1].
PML_PLAN std::string pml_plan_time_segments(const int* parent, const double* node_time, int N, const double* boundaries, int M,
                                            PmlTimeSegments& out);

// The pieces the device sums over: at most `piece` consecutive segments, cut per bin so that no piece straddles two bins.
// piece_off [pieces + 1]: piece p holds the segments [piece_off[p], piece_off[p + 1]); bin_piece_off [bins + 1]: the pieces of
// bin m, in order.  with_points: the pseudo-bin M is cut as well (bins = M + 1), else the pieces end with bin M - 1 (bins = M).
struct PmlTimePieces {
    std::vector<int> piece_off, bin_piece_off;
    int n_pieces() const { return piece_off.empty() ? 0 : (int)piece_off.size() - 1; }
};
PML_PLAN PmlTimePieces pml_cut_time_pieces(const PmlTimeSegments& plan, int piece, bool with_points);

// The upper ends of the segments, for what places points on a branch (pml_sample_histories_through_time): s2 of a segment is
// the s1 of the same branch's segment in the next bin -- the same quotient (T_{m+1} - time_p) / h, hence the same double --,
// for a branch that leaves the range the s1 of its point segment at T_M.  Where the branch ends inside the bin (no segment in
// the next bin: r == 0, every h == 0 branch, every point segment) s2 = 1 and `ends` is set: the end belongs to the segment.  The
// segments of a branch then tile it without gap or overlap, in bits: a point c lies in the one segment with s1 <= c < s2 (or,
// with `ends`, s1 <= c).  Never s1 + w or 1 - r: neighbours would disagree by an ulp.  From the plan alone.
struct PmlTimeSegmentEnds {
    std::vector<double> s2;   // [segments]
    std::vector<int> ends;    // [segments]
};
PML_PLAN PmlTimeSegmentEnds pml_time_segment_ends(const PmlTimeSegments& plan);
