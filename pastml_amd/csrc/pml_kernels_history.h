// Exact expected dwell times and Markov jumps along the tree for the F81 family (F81 / JC / EFT), all columns of a call in one
// pass (pml_expected_history): the posterior mean, over whole histories, of the time spent in each state and of the number of
// jumps i -> j -- events, not end-point differences (pml_kernels_expected.h counts those).
//
// Per column and non-root node n with parent p, in the notation of pml_kernels_gradient.h: mu = 1 / (1 - pi . pi),
// t'_n = (d_n + tau) tf sf, L_n = (d_n + tau) tf, x_n = mu t'_n, e_n = exp(-x_n), v_n the bottom-up vector of n (a tip: its 0/1
// mask; any scaling cancels), S_n = pi . v_n, m_n[i] = (1 - e_n) S_n + e_n v_n[i], q_p the marginal posterior of p,
// o_n[i] = q_p[i] / m_n[i] (0 where q_p[i] == 0), O_n = sum_i o_n[i].  With
//     g = (1 - e) / x,   c0 = 1 - 2 g + e,   c1 = g - e                                (all >= 0; g = 1, c0 = c1 = 0 at x = 0)
//     a_n[i] = pi_i O_n S_n c0 + o_n[i] S_n c1,     b_n[i] = pi_i O_n c1 + o_n[i] e_n
// the posterior share of branch n spent in state s is f_n[s] = a_n[s] + b_n[s] v_n[s] (sum_s f_n[s] = 1), the expected number
// of jumps i -> j on it is J_n[i][j] = x_n pi_j (a_n[i] + b_n[i] v_n[j]) for i != j, and
//     times[s]        = sum_n L_n f_n[s]
//     jumps[i][j]     = pi_j (sum_n x_n a_n[i]  +  sum_n x_n b_n[i] v_n[j])             (i != j; the diagonal is 0)
//     branch_jumps[n] = x_n sum_i (a_n[i] (1 - pi_i) + b_n[i] (S_n - pi_i v_n[i]))      (= sum_{i != j} J_n[i][j]; a root: 0)
// Every term is non-negative.  A branch with t' = 0 adds nothing.
//
// history_branch_kernel streams v_n and q_p once per branch (2 k doubles, as gradient_f81_kernel does) and leaves the pieces'
// partial times and sum x a; history_jump_kernel forms sum_n (x_n b_n) (x) v_n on the FP64 matrix cores
// (hist_jump_product); history_vector_kernel and history_matrix_kernel sum the partials in piece order.  The arguments, the
// coefficients, the front half of the branch pass, the units' sums, the product and the piece sums are
// pml_kernels_history_shared.h's, which the sums per time interval (pml_kernels_history_time.h) share.
//
// b_n in the product.  It is formed again there, not staged: the branch pass leaves three doubles per branch and column -- S_n,
// x_n O_n c1 and x_n e_n, 24 bytes written and read once per tile group -- and the product forms
// x_n b_n[i] = pi_i (x_n O_n c1) + o_n[i] (x_n e_n) from the q_p and v_n it streams anyway (one division per element, no
// exponential).  Staging x_n b_n itself would be 8 k bytes per branch and column written and read: half as much again as the
// 16 k bytes the branch pass streams.
//
// 1 - e and e.  In m_n it is 1.0 - e_n with the stored e_n, as the sweeps formed it: q_p carries m_n as a factor, and
// q_p[i] / m_n[i] is that factor cancelled only if both are the same number (pml_kernels_gradient.h).  The explicit e_n, g, c0
// and c1 are formed from x_n: for x < 1 by  c1 = e sum_{m >= 1} x^m / (m + 1)!,  c0 = e sum_{m >= 2} x^m (m - 1) / (m + 1)!
// (the series of the header times e^x e^-x: every term positive, no cancellation; 1 - 2 g + e formed directly has no digit left
// at x = 1e-9), from expm1 otherwise.
//
// Bits.  No floating-point atomics.  The nodes are walked in the CALLER's numbering and cut into pieces of a fixed number of
// ids (a function of k only, one size for the branch pass and one for the product); a workgroup owns one piece (and tile
// group), the units of the branch pass take the ids of the piece round robin and their sums are combined through LDS in unit
// order, and the partials are summed in piece order.  Nothing depends on the grid, on the schedule of the sweeps, on the
// library's own numbering or on the column.
#pragma once
#include "pml_kernels_history_shared.h"

// The branch pass (the lane shapes: pml_kernels_history_shared.h).  grid (piece, column).
template <int G, int R>
__global__ void __launch_bounds__(256) history_branch_kernel(PmlHistArgs A) {
    constexpr int U = 64 / G, UNITS = 4 * U;
    __shared__ double red[UNITS * 2 * G * R];
    const int lane = threadIdx.x & 63, g = lane % G;
    const int unit = (threadIdx.x >> 6) * U + lane / G;
    const HistColumn<R> C = hist_column<G, R>(A, A.col0 + blockIdx.y, g);
    double acc_t[R], acc_a[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc_t[r] = acc_a[r] = 0.0;
    const int i0 = blockIdx.x * A.piece, i1 = min(A.N, i0 + A.piece);
    for (int base = i0; base < i1; base += UNITS) {   // (the same trip count in every unit: the lane exchanges below are convergent)
        const int i = min(base + unit, i1 - 1);
        const bool inside = base + unit < i1;
        const int n = A.new_of_old ? A.new_of_old[i] : i;
        const int p = A.parent[n];
        const bool branch = inside && p >= 0;
        const double d = A.dist[n] + C.tau;
        const double x = branch ? C.mu * (d * C.scale) : 0.0;   // (the transform of f81_prep_kernel)
        const double len = branch ? d * C.tauf : 0.0;
        double v[R], o[R], s, o_sum;
        hist_front<G, R>(A, C, g, n, p, branch, v, o, s, o_sum);
        double e, c0, c1;
        hist_coefficients(x, e, c0, c1);
        const double os0 = o_sum * s * c0, sc1 = s * c1, oc1 = o_sum * c1;
        double bj = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double a = C.pi[r] * os0 + o[r] * sc1;
            const double b = C.pi[r] * oc1 + o[r] * e;
            acc_t[r] += len * (a + b * v[r]);
            acc_a[r] += x * a;
            bj += a * (1.0 - C.pi[r]) + b * (s - C.pi[r] * v[r]);
        }
        bj = group_sum<G>(bj);
        if (g == 0 && inside) {
            if (A.branch_out != nullptr) A.branch_out[(size_t)blockIdx.y * A.N + i] = x * bj;
            if (A.stage != nullptr) {
                double* st = A.stage + ((size_t)blockIdx.y * A.N + n) * 3;
                st[0] = s;
                st[1] = x * oc1;
                st[2] = x * e;
            }
        }
    }
    hist_unit_sums<G, R>(red, unit, g, A.k, A.partial + ((size_t)blockIdx.y * A.n_pieces + blockIdx.x) * 2 * A.k, acc_t, acc_a);
}

// times and sum x a: the pieces' partials in piece order.  grid (column); thread t owns the entries t + 256 h of the 2 k <= 1024.
static __global__ void __launch_bounds__(256) history_vector_kernel(PmlHistArgs A) {
    const int k = A.k;
    const double* part = A.partial + (size_t)blockIdx.x * A.n_pieces * 2 * k;
    for (int t = threadIdx.x; t < 2 * k; t += 256) {
        const double s = pml_piece_sum(part + t, (size_t)2 * k, 0, A.n_pieces);
        if (t < k) A.times_out[(size_t)blockIdx.x * k + t] = s;
        else A.xa[(size_t)blockIdx.x * k + (t - k)] = s;
    }
}

// sum_n (x_n b_n) (x) v_n of one piece of ids: item i is the node with the caller's id i, its staged scalars are kept by node,
// and a root adds nothing.  grid (piece, tile group, column)
struct HistNodeItems {
    const int* new_of_old;
    __device__ __forceinline__ void at(int i, int& n, int& stage_row) const { stage_row = n = new_of_old ? new_of_old[i] : i; }
    __device__ __forceinline__ bool valid(bool inside, int p) const { return inside && p >= 0; }
};
template <int WIDE>
__global__ void __launch_bounds__(256) history_jump_kernel(PmlHistArgs A) {
    const int i0 = blockIdx.x * A.jpiece;
    hist_jump_product<WIDE>(A, HistNodeItems{A.new_of_old}, A.stage + (size_t)blockIdx.z * A.N * 3, i0, min(A.N, i0 + A.jpiece),
                            A.jpartial + ((size_t)blockIdx.z * A.n_jpieces + blockIdx.x) * A.k * A.k);
}

// jumps[col][i][j]: hist_jumps_entry over all pieces.  grid (k k / 256, column)
static __global__ void __launch_bounds__(256) history_matrix_kernel(PmlHistArgs A) {
    const int k = A.k;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= k * k) return;
    A.jumps_out[(size_t)blockIdx.y * k * k + idx] = hist_jumps_entry(A, blockIdx.y, idx, A.jpartial + (size_t)blockIdx.y * A.n_jpieces * k * k,
                                                                     0, A.n_jpieces, A.xa + (size_t)blockIdx.y * k);
}
