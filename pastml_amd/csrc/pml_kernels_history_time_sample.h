// Stochastic character maps of the F81 family cut at the boundaries of time bins (pml_sample_histories_through_time): the
// histories of pml_kernels_history_sample.h -- the same scenarios, the same draws, the same event counts, exponentials and
// states --, placed on their branches and binned by the segment plan of pml_time_segments.h.  pml_kernels_history_time.h gives
// the means of what is drawn here in closed form.
//
// The law.  Repetition g of node n has M events, the exponentials w_0 .. w_M, their sum Wsum (left to right) and the states
// s_0 = a, .., s_M = b exactly as there (steps 1 - 3 of its header; Philox counter (g, caller's id, d >> 2, PML_HSAMP_TAG)).  New:
//   positions.  c_0 = 0; P_i = w_0 + .. + w_{i-1} left to right, c_i = P_i / Wsum for i = 1 .. M; c_{M+1} = 1 (set, not computed).
//      History interval i is [c_i, c_{i+1}) in state s_i; event i >= 1 happens at c_i.  The c_i do not descend.
//   segments.  Those of pml_plan_time_segments (s1, w, starts, the pseudo-bin M) with the upper ends of pml_time_segment_ends: s2
//      the s1 of the branch's segment in the next bin, or 1 with `ends` where the branch ends in the bin.  A point c belongs to the
//      one segment with s1 <= c < s2 (with `ends`: s1 <= c).
//   dwell.  Interval i gives segment (n, m) the time L_n w -- the plan's own w -- if c_i <= s1 and s2 <= c_{i+1}; otherwise
//      lo = max(c_i, s1), hi = min(c_{i+1}, s2), v = hi - lo and, where v > 0, L_n v.  It is added to times[g][m][s_i].  M = 0: the
//      one interval [0, 1) in state a, L_n w with no draw beyond draw 0.
//   jumps.  Event i >= 1 with s_{i-1} != s_i whose c_i belongs to segment (n, m) adds 1 to jumps[g][m][s_{i-1}][s_i].
//   lineages.  Every segment with `starts` (those of the pseudo-bin M included) adds 1 to lineages[g][m][s_i] for the largest i
//      with c_i <= s1: an event exactly at the boundary has happened, and a branch that begins there (s1 == 0) shows a.
// Every operation is a statement of its own (no contraction into an FMA): tests/history_time_sample_ref.py restates them.
// A branch with x_n > PML_HSAMP_MAX_X is not drawn; htsamp_count_kernel counts those of the whole forest and the call fails.
//
// Bits.  No floating-point atomics.  The segments are sorted by (bin, caller's id) and cut into pieces of a number of segments
// that depends on N only and that never straddle two bins (pml_cut_time_pieces); a workgroup takes one (piece, tile of
// repetitions), a thread owns one repetition, walks the piece's segments in order and adds to accumulators it owns alone:
// hsamp_kernel's, acc[state][repetition] in LDS up to PML_HSAMP_LDS_K states, beyond that its own row of the partials in HBM.
// htsamp_sum_kernel adds a bin's pieces in piece order: the rows of a bin do not depend on the other bins.  jumps and lineages
// are integers (atomic adds commute).
//
// Cost.  The generator is counter-based, so a thread derives the history of a branch afresh for every segment: draw 0 and the
// event count; only if there are events Wsum, and then the walk, which draws a state only from the first interval that reaches
// s1 and stops behind s2.  A branch that spans B bins is derived B times.
#pragma once
#include "pml_kernels_history_sample.h"

#define PML_HTSAMP_STARTS 1
#define PML_HTSAMP_ENDS 2

struct PmlHtsampArgs {
    const int* parent;          // the library's numbering, as dist and E
    const int* new_of_old;      // caller's id -> library's id; null = the same
    const int* old_of_new;      // library's id -> caller's id; null = the same
    const double* dist;         // [N]
    const double* pi;           // [ks] of the column
    const double* E;            // [N] of the column
    const double *mu, *sf, *tau, *tauf;   // the column's entries
    int N, k, M;
    const int* seg_node;        // [segments] caller's id
    const int* seg_flags;       // [segments] PML_HTSAMP_STARTS | PML_HTSAMP_ENDS
    const double* seg_pos;      // [segments][3]: s1, w, s2
    const int* piece_off;       // [n_pieces + 1]
    const int* piece_bin;       // [n_pieces]; the pieces of the pseudo-bin M (lineages only) come last
    const int* bin_piece_off;   // [M + 1]: the pieces of the bins proper
    int n_pieces, n_sum_pieces;
    int n_tiles;                // tiles of blockDim.x repetitions
    int n_rep;
    size_t rs;                  // row stride of states (elements)
    const void* states;         // [N][rs], caller's numbering (uint8 up to 256 states, else uint16)
    unsigned rep_offset;
    u64 seed;
    double* partial;            // [n_sum_pieces][n_rep][k] (beyond PML_HSAMP_LDS_K states: zeroed, the accumulators themselves)
    double* times_out;          // [n_rep][M][k]
    unsigned* jumps;            // [n_rep][M][k][k], zeroed, or null
    unsigned* lineages;         // [n_rep][M + 1][k], zeroed, or null
    unsigned long long* n_skipped;   // branches with x > PML_HSAMP_MAX_X (zeroed)
};

// step 1 of pml_kernels_history_sample.h, statement for statement (hsamp_kernel holds it inline): the number of events of a
// branch with x != 0 whose ends are in the states a and b; u = draw 0, pa = pi[a]
__device__ __forceinline__ int htsamp_events(double x, double e, bool same, double pa, double u) {
    const double q = 1.0 - e;
    double target = 0.0;
    if (!same) {
        target = u * q;
    } else {
        const double qa = q * pa;
        const double Wa = qa + e;
        const double t = u * Wa;
        if (t < e) return 0;
        const double rest = t - e;
        target = rest / pa;
    }
    double term = e * x;
    double cum = term;
    int m = 1;
    while (cum <= target) {
        m += 1;
        const double tx = term * x;
        term = tx / (double)m;
        const double next = cum + term;
        if (next == cum || m == PML_HSAMP_MAX_EVENTS) break;
        cum = next;
    }
    return m;
}

// grid: n_pieces * n_tiles workgroups of blockDim.x (a multiple of 64) threads.  Dynamic LDS: pi [k], its cumulative table [k],
// then (!WIDE) the accumulators [k][blockDim.x + 1].
template <bool WIDE>
__global__ void __launch_bounds__(256) htsamp_kernel(PmlHtsampArgs A) {
    typedef typename std::conditional<WIDE, unsigned short, unsigned char>::type T;
    extern __shared__ double htsamp_lds[];
    const int k = A.k;
    const int tid = threadIdx.x, Tt = blockDim.x;
    double* pil = htsamp_lds;
    double* pcdf = htsamp_lds + k;
    for (int b = tid; b < k; b += Tt) pil[b] = A.pi[b];
    if (tid < 64) {   // (the simulator's table)
        double run = 0.0;
        for (int b0 = 0; b0 < k; b0 += 64) {
            const int b = b0 + tid;
            const double inc = sim_wave_scan(b < k ? A.pi[b] : 0.0, tid) + run;
            if (b < k) pcdf[b] = inc;
            run = __shfl(inc, 63, 64);
        }
    }
    const int piece = blockIdx.x / A.n_tiles, tile = blockIdx.x % A.n_tiles;
    const int bin = A.piece_bin[piece];
    const bool point = bin == A.M;   // the pseudo-bin: lineages only, no accumulators
    const int r = tile * Tt + tid;
    const bool active = r < A.n_rep;
    // the accumulator of state s: acc[s * as]
    double* acc;
    int as;
    if (WIDE) {
        acc = point ? A.partial : A.partial + ((size_t)piece * A.n_rep + min(r, A.n_rep - 1)) * k;
        as = 1;
    } else {
        acc = htsamp_lds + 2 * k + tid;
        as = Tt + 1;
        if (!point)
            for (int s = 0; s < k; ++s) acc[s * as] = 0.0;
    }
    __syncthreads();
    const double ptotal = pcdf[k - 1];
    const double mu = A.mu[0], tau = A.tau[0], tauf = A.tauf[0];
    const double scale = tauf * A.sf[0];
    const T* states = reinterpret_cast<const T*>(A.states);
    if (active) {
        const unsigned g = A.rep_offset + (unsigned)r;
        unsigned* jumps = A.jumps == nullptr ? nullptr : A.jumps + ((size_t)r * A.M + (point ? 0 : bin)) * k * k;
        unsigned* lineages = A.lineages == nullptr ? nullptr : A.lineages + ((size_t)r * (A.M + 1) + bin) * k;
        const int i0 = A.piece_off[piece], i1 = A.piece_off[piece + 1];
        for (int seg = i0; seg < i1; ++seg) {
            const int id = A.seg_node[seg];
            const int flags = A.seg_flags[seg];
            const bool starts = (flags & PML_HTSAMP_STARTS) != 0 && lineages != nullptr;
            const bool ends = (flags & PML_HTSAMP_ENDS) != 0;
            if (point && !starts) continue;
            const int n = A.new_of_old ? A.new_of_old[id] : id;
            const int p = A.parent[n];
            if (p < 0) continue;
            const double d = A.dist[n] + tau;
            const double dt = d * scale;
            const double x = mu * dt;   // (the transform of pml_kernels_history.h)
            const double L = d * tauf;
            if (x > PML_HSAMP_MAX_X) continue;
            const double s1 = A.seg_pos[3 * (size_t)seg], w = A.seg_pos[3 * (size_t)seg + 1], s2 = A.seg_pos[3 * (size_t)seg + 2];
            const int pid = A.old_of_new ? A.old_of_new[p] : p;
            const int a = (int)states[(size_t)pid * A.rs + r];
            const int b = (int)states[(size_t)id * A.rs + r];
            HsampDraws draws(A.seed, g, (unsigned)id);
            int M = 0;
            if (x != 0.0) M = htsamp_events(x, A.E[n], a == b, pil[a], sim_u(draws.word(0u)));
            if (M == 0) {
                if (!point) {
                    const double whole = L * w;
                    acc[a * as] += whole;
                }
                if (starts) atomicAdd(&lineages[a], 1u);
                continue;
            }
            double Wsum = 0.0;
            for (int i = 0; i <= M; ++i) {
                const double wi = hsamp_exponential(draws.word(1u + (unsigned)i));
                Wsum += wi;
            }
            HsampDraws redraws(A.seed, g, (unsigned)id);
            double P = 0.0, c_lo = 0.0;
            int prev = a, at_start = a;
            for (int i = 0; i <= M; ++i) {
                // behind the segment: no dwell, no event and no boundary state from here on
                if (c_lo > s1 && (point || (!ends && c_lo >= s2))) break;
                const double wi = hsamp_exponential(draws.word(1u + (unsigned)i));
                const double Pn = P + wi;
                double c_hi = 1.0;
                if (i < M) c_hi = Pn / Wsum;
                P = Pn;
                if (c_hi < s1) {   // before the segment, its event as well: the state is not needed
                    c_lo = c_hi;
                    continue;
                }
                int s = a;
                if (i == M) {
                    s = b;
                } else if (i > 0) {
                    const double us = sim_u(redraws.word((unsigned)(M + 1 + i)));
                    const double at = us * ptotal;
                    s = sim_bisect(pcdf, k, at);
                }
                if (!point) {
                    if (c_lo <= s1 && s2 <= c_hi) {
                        const double whole = L * w;
                        acc[s * as] += whole;
                    } else {
                        const double lo = fmax(c_lo, s1);
                        const double hi = fmin(c_hi, s2);
                        const double v = hi - lo;
                        if (v > 0.0) {
                            const double part = L * v;
                            acc[s * as] += part;
                        }
                    }
                    if (i > 0 && s != prev && jumps != nullptr && c_lo >= s1 && (ends || c_lo < s2))
                        atomicAdd(&jumps[(size_t)prev * k + s], 1u);
                }
                if (c_lo <= s1) at_start = s;
                prev = s;
                c_lo = c_hi;
            }
            if (starts) atomicAdd(&lineages[at_start], 1u);
        }
    }
    if (!WIDE && !point) {
        // the tile's accumulators, transposed: consecutive lanes write consecutive states of a repetition
        __syncthreads();
        const int r0 = tile * Tt, nr = min(Tt, A.n_rep - r0);
        double* out = A.partial + ((size_t)piece * A.n_rep + r0) * k;
        const double* all = htsamp_lds + 2 * k;
        for (int idx = tid; idx < nr * k; idx += Tt) {
            const int rr = idx / k, s = idx - rr * k;
            out[idx] = all[s * (Tt + 1) + rr];
        }
    }
}

// times[r][m][s]: the partials of the pieces of bin m in piece order (an empty bin: exact zeros).  One thread per entry.
static __global__ void __launch_bounds__(256) htsamp_sum_kernel(PmlHtsampArgs A) {
    const size_t total = (size_t)A.n_rep * A.M * A.k;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t s = idx % A.k, rm = idx / A.k;
    const size_t m = rm % A.M, r = rm / A.M;
    double sum = 0.0;
    for (int j = A.bin_piece_off[m]; j < A.bin_piece_off[m + 1]; ++j) sum += A.partial[((size_t)j * A.n_rep + r) * A.k + s];
    A.times_out[idx] = sum;
}

// the branches of the forest with x > PML_HSAMP_MAX_X.  One thread per node of the library's numbering.
static __global__ void __launch_bounds__(256) htsamp_count_kernel(PmlHtsampArgs A) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= A.N || A.parent[n] < 0) return;
    const double d = A.dist[n] + A.tau[0];
    const double scale = A.tauf[0] * A.sf[0];
    const double dt = d * scale;
    const double x = A.mu[0] * dt;
    if (x > PML_HSAMP_MAX_X) atomicAdd(A.n_skipped, 1ull);
}
