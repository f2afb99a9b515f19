// Stochastic character maps of the F81 family (F81 / JC / EFT) drawn on the device (pml_sample_histories): given a scenario of
// the joint posterior (pml_kernels_scenarios.h: one state per node and repetition), a whole history on every branch -- the
// events between the two end states and the time spent in each state.  pml_kernels_history.h gives the means of what is drawn
// here in closed form.
//
// The law.  Q = mu (1 pi^T - I) is a Poisson process of rate mu whose events redraw the state from pi (an event may redraw
// the state it finds: a virtual event).  In the notation of pml_kernels_history.h -- mu = 1 / (1 - pi . pi),
// t'_n = (d_n + tau) tf sf, L_n = (d_n + tau) tf, x_n = mu t'_n formed as there, e_n the STORED E[n] the scenario sampler used --
// and for repetition g and non-root node n whose parent is in state a and which is in state b itself:
//   1. the number of events M.  x_n == 0: M = 0.  Otherwise q = 1.0 - e_n, u = draw 0;  a != b: target = u q;
//      a == b: Wa = q pi[a] + e_n, t = u Wa, M = 0 if t < e_n, else target = (t - e_n) / pi[a].  M >= 1 by inversion over the
//      terms e x^m / m!:   term = e_n x_n; cum = term; m = 1;
//                          while cum <= target: m += 1; term = (term x_n) / m; if cum + term == cum or m == MAX_EVENTS: stop;
//                                               cum += term
//      (a zero-truncated Poisson; with equal ends the mass e_n / Wa at zero).
//   2. the spacings.  M >= 1: draws 1 .. M + 1 give w_i = -log((X_i + 0.5) 2^-32), i = 0 .. M (X the 32-bit word: no uniform is
//      0), Wsum their sum left to right, dwell_i = (L_n w_i) / Wsum: normalised iid exponentials are the spacings of M uniform
//      order statistics -- no sort, no pow.  Two passes over the same counters (the generator is counter-based).  M = 0: the
//      whole L_n goes to a, no draw.
//   3. the states.  s_0 = a, s_M = b, draws M + 2 .. 2 M give s_1 .. s_{M-1}: sim_bisect of the column's sim_wave_scan table of
//      pi at u times the table's last entry, u = X 2^-32.  Interval i adds dwell_i to times[g][s_i]; every i >= 1 with
//      s_{i-1} != s_i adds 1 to jumps[g][s_{i-1}][s_i] and to branch_jumps[n][g].  Virtual events count nowhere.
// Draw d of (node, global repetition g = rep_offset + r) is word d & 3 of Philox-4x32-10 keyed by the seed with the counter
// (g, caller's node id, d >> 2, PML_HSAMP_TAG): the result is a pure function of (seed, node, global repetition).
// A branch with x_n > PML_HSAMP_MAX_X is not drawn (e_n leaves the normal doubles there and the inversion its meaning): it is
// counted, and the call fails.
// Every operation above is a statement of its own (no contraction into an FMA), so that the arithmetic can be restated
// operation by operation (tests/history_sample_ref.py).
//
// Bits.  The rule of pml_kernels_history.h: no floating-point atomics.  The nodes are walked in the CALLER's numbering and cut
// into pieces of a number of ids that depends on N only; a workgroup takes one (piece, tile of repetitions), a thread owns one
// repetition, walks the piece's ids in ascending order and adds each dwell, event by event, to accumulators it owns alone:
// up to PML_HSAMP_LDS_K states acc[state][repetition] in LDS (rows of blockDim.x + 1 doubles: lanes that hit the same state sit
// in consecutive banks, and the transposed read at the end of the piece does not conflict either), beyond that its own row of
// the partials in HBM.  hsamp_sum_kernel adds the pieces' partials [piece][rep][k] in piece order.  The jumps are integers
// (atomic adds commute); a branch count has one owner.
#pragma once
#include <type_traits>
#include "pml_kernels_simulate.h"

#define PML_HSAMP_TAG 0x68697374u   // word 3 of the counter (the simulator's, the scenario sampler's and the counts sampler's: others)
#define PML_HSAMP_MAX_EVENTS 4096
#define PML_HSAMP_MAX_X 512.0
#define PML_HSAMP_LDS_K 256

struct PmlHsampArgs {
    const int* parent;          // the library's numbering, as dist and E
    const int* new_of_old;      // caller's id -> library's id; null = the same
    const int* old_of_new;      // library's id -> caller's id; null = the same
    const double* dist;         // [N]
    const double* pi;           // [ks] of the column
    const double* E;            // [N] of the column
    const double *mu, *sf, *tau, *tauf;   // the column's entries
    int N, k;
    int piece, n_pieces;        // ids per piece
    int n_tiles;                // tiles of blockDim.x repetitions
    int n_rep;
    size_t rs;                  // row stride of states (elements)
    const void* states;         // [N][rs], caller's numbering (uint8 up to 256 states, else uint16)
    unsigned rep_offset;
    u64 seed;
    double* partial;            // [n_pieces][n_rep][k] (beyond PML_HSAMP_LDS_K states: zeroed, the accumulators themselves)
    double* times_out;          // [n_rep][k]
    unsigned* jumps;            // [n_rep][k][k], zeroed, or null
    unsigned short* branch;     // [N][n_rep], caller's numbering, or null
    unsigned long long* n_skipped;   // branches with x > PML_HSAMP_MAX_X (zeroed)
};

// the draws of one (node, repetition): the block of four words that holds draw d is formed when d leaves the one held.  The
// four words are kept as two 64-bit values and picked by shifts: an array indexed by d & 3 would live in private memory.
struct HsampDraws {
    unsigned k0, k1, g, key, block;
    u64 lo, hi;   // words 0, 1 and 2, 3 of the block
    __device__ __forceinline__ HsampDraws(u64 seed, unsigned g_, unsigned key_)
        : k0((unsigned)seed), k1((unsigned)(seed >> 32)), g(g_), key(key_), block(0xffffffffu), lo(0), hi(0) {}
    __device__ __forceinline__ unsigned word(unsigned d) {
        const unsigned blk = d >> 2;
        if (blk != block) {
            unsigned c[4] = {g, key, blk, PML_HSAMP_TAG};
            philox4x32_10(c, k0, k1);
            lo = (u64)c[0] | ((u64)c[1] << 32);
            hi = (u64)c[2] | ((u64)c[3] << 32);
            block = blk;
        }
        const u64 pair = (d & 2u) ? hi : lo;
        return (unsigned)(pair >> ((d & 1u) * 32u));
    }
};

// an exponential variate from a 32-bit word
__device__ __forceinline__ double hsamp_exponential(unsigned x) {
    const double h = (double)x + 0.5;
    const double u = h * 0x1p-32;
    return -log(u);
}

// grid: n_pieces * n_tiles workgroups of blockDim.x (a multiple of 64) threads.  Dynamic LDS: pi [k], its cumulative table [k],
// then (!WIDE) the accumulators [k][blockDim.x + 1].
template <bool WIDE>
__global__ void __launch_bounds__(256) hsamp_kernel(PmlHsampArgs A) {
    typedef typename std::conditional<WIDE, unsigned short, unsigned char>::type T;
    extern __shared__ double hsamp_lds[];
    const int k = A.k;
    const int tid = threadIdx.x, Tt = blockDim.x;
    double* pil = hsamp_lds;
    double* pcdf = hsamp_lds + k;
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
    const int r = tile * Tt + tid;
    const bool active = r < A.n_rep;
    // the accumulator of state s: acc[s * as]
    double* acc;
    int as;
    if (WIDE) {
        acc = A.partial + ((size_t)piece * A.n_rep + min(r, A.n_rep - 1)) * k;
        as = 1;
    } else {
        acc = hsamp_lds + 2 * k + tid;
        as = Tt + 1;
        for (int s = 0; s < k; ++s) acc[s * as] = 0.0;
    }
    __syncthreads();
    const double ptotal = pcdf[k - 1];
    const double mu = A.mu[0], tau = A.tau[0], tauf = A.tauf[0];
    const double scale = tauf * A.sf[0];
    const T* states = reinterpret_cast<const T*>(A.states);
    unsigned skipped = 0;
    if (active) {
        const unsigned g = A.rep_offset + (unsigned)r;
        const int i0 = piece * A.piece, i1 = min(A.N, i0 + A.piece);
        for (int id = i0; id < i1; ++id) {
            const int n = A.new_of_old ? A.new_of_old[id] : id;
            const int p = A.parent[n];
            unsigned bj = 0;
            if (p >= 0) {
                const double d = A.dist[n] + tau;
                const double dt = d * scale;
                const double x = mu * dt;   // (the transform of pml_kernels_history.h)
                const double L = d * tauf;
                if (x > PML_HSAMP_MAX_X) {
                    skipped += r == 0;
                } else {
                    const int pid = A.old_of_new ? A.old_of_new[p] : p;
                    const int a = (int)states[(size_t)pid * A.rs + r];
                    const int b = (int)states[(size_t)id * A.rs + r];
                    HsampDraws draws(A.seed, g, (unsigned)id);
                    int M = 0;
                    if (x != 0.0) {
                        const double e = A.E[n];
                        const double q = 1.0 - e;
                        const double u = sim_u(draws.word(0u));
                        double target = 0.0;
                        bool none = false;
                        if (a != b) {
                            target = u * q;
                        } else {
                            const double pa = pil[a];
                            const double qa = q * pa;
                            const double Wa = qa + e;
                            const double t = u * Wa;
                            if (t < e) {
                                none = true;
                            } else {
                                const double rest = t - e;
                                target = rest / pa;
                            }
                        }
                        if (!none) {
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
                            M = m;
                        }
                    }
                    if (M == 0) {
                        acc[a * as] += L;
                    } else {
                        double Wsum = 0.0;
                        for (int i = 0; i <= M; ++i) {
                            const double w = hsamp_exponential(draws.word(1u + (unsigned)i));
                            Wsum += w;
                        }
                        HsampDraws redraws(A.seed, g, (unsigned)id);
                        int prev = a;
                        for (int i = 0; i <= M; ++i) {
                            const double w = hsamp_exponential(draws.word(1u + (unsigned)i));
                            const double lw = L * w;
                            const double dwell = lw / Wsum;
                            int s = a;
                            if (i == M) {
                                s = b;
                            } else if (i > 0) {
                                const double us = sim_u(redraws.word((unsigned)(M + 1 + i)));
                                const double at = us * ptotal;
                                s = sim_bisect(pcdf, k, at);
                            }
                            acc[s * as] += dwell;
                            if (i > 0 && s != prev) {
                                ++bj;
                                if (A.jumps != nullptr) atomicAdd(&A.jumps[((size_t)r * k + prev) * k + s], 1u);
                            }
                            prev = s;
                        }
                    }
                }
            }
            if (A.branch != nullptr) A.branch[(size_t)id * A.n_rep + r] = (unsigned short)bj;
        }
    }
    if (!WIDE) {
        // the tile's accumulators, transposed: consecutive lanes write consecutive states of a repetition
        __syncthreads();
        const int r0 = tile * Tt, nr = min(Tt, A.n_rep - r0);
        double* out = A.partial + ((size_t)piece * A.n_rep + r0) * k;
        const double* all = hsamp_lds + 2 * k;
        for (int idx = tid; idx < nr * k; idx += Tt) {
            const int rr = idx / k, s = idx - rr * k;
            out[idx] = all[s * (Tt + 1) + rr];
        }
    }
    if (skipped) atomicAdd(A.n_skipped, (unsigned long long)skipped);
}

// times[r][s]: the pieces' partials in piece order.  One thread per entry.
static __global__ void __launch_bounds__(256) hsamp_sum_kernel(PmlHsampArgs A) {
    const size_t total = (size_t)A.n_rep * A.k;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    double s = 0.0;
    for (int j = 0; j < A.n_pieces; ++j) s += A.partial[(size_t)j * total + idx];
    A.times_out[idx] = s;
}
