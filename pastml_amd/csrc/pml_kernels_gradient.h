// Exact gradient of ln L for the F81 family (F81 / JC / EFT), all columns of a call in one pass (pml_loglik_gradient).
//
// The likelihood is multilinear in the per-branch matrices P_n = (1 - e_n) 1 pi^T + e_n I, e_n = exp(-mu t'_n),
// t'_n = (d_n + tau) tf sf, mu = 1 / (1 - pi . pi).  With v_n the bottom-up vector of n (a tip: its 0/1 mask; any scaling
// cancels), s_n = pi . v_n, the message m_n[i] = (1 - e_n) s_n + e_n v_n[i] and q_p the marginal posterior of n's parent,
// d ln L / d m_n[i] = q_p[i] / m_n[i].  So, per non-root n with e_n < 1:
//     A_n = sum_i q_p[i] / m_n[i]          (terms with q_p[i] == 0 are zero)
//     B_n = sum_i q_p[i] v_n[i] / m_n[i]
//     h_n = -mu e_n (B_n - s_n A_n)                                                  (= d ln L / d t'_n)
//     T0 = sum_n h_n,  T1 = sum_n h_n t'_n,  E[m] = sum_n (1 - e_n) A_n v_n[m] + sum over the roots r of v_r[m] / (pi . v_r)
// and  d/d sf = T1 / sf,  d/d tau at fixed tf = T0 tf sf,  d/d tf = T1 / tf,  d/d pi_m = E[m] + 2 mu pi_m T1  (pi_m free; mu's
// dependence on pi included).  Nothing is swept: the pass streams the posterior rows, the bottom-up rows and e_n that the marginal
// pass left on the device -- what pml_kernels_expected.h reads.
//
// 1 - e.  In m_n it is 1.0 - e_n with the stored e_n, as the sweeps formed it: q_p carries m_n as a factor, and q_p[i] / m_n[i]
// is that factor cancelled only if both are the same number (on a branch of 1e-12 the two ways differ by 1e-4 of 1 - e).  The
// explicit factor (1 - e_n) of E is -expm1(-mu t'_n).
// A branch whose e_n is 1.0 as a double (t' = 0, or below 1e-16) is flat: its factors t' and 1 - e vanish from T1 and E, its
// share of T0 cannot be recovered from stored posteriors (q_p[i] / m_n[i] is 0 / 0 on the states v_n excludes).  Such branches
// are left out and counted (n_flat): the tau component is valid only where the count is zero.
//
// Bits.  No floating-point atomics.  The nodes are walked in the CALLER's numbering and cut into pieces of a fixed number of
// ids (a function of k only); a workgroup owns one piece, its units take the ids of the piece round robin, their sums are
// combined through LDS in unit order, and gradient_reduce_kernel sums the pieces' partials in piece order.  Nothing depends on
// the grid, on the schedule of the sweeps, on the library's own numbering or on the column.
#pragma once
#include "pml_device.h"

struct PmlGradArgs {
    const int* parent;              // the library's numbering, as all per-node arrays below
    const int* n_children;
    const int* new_of_old;          // caller's id -> library's id; null = the same
    const double* dist;             // [N]
    const u64* masks;               // [C][N][W]
    const double* pi;               // [C][ks]
    const double* bu;               // [C][N][ks]   (tips: not stored, their masks as 0/1)
    const double* post;             // [C][N][ks]
    const double* E;                // [C][N]
    const double *mu, *sf, *tau, *tauf;   // [C]
    int N, k, ks, W;
    int col0;                       // first column of the call; blockIdx.y counts from it
    int piece, n_pieces;            // ids per piece
    double* partial;                // [cols][n_pieces][k + 3]: T0, T1, n_flat, E[0..k)
    double* rates_out;              // [cols][3]: d/d sf, d/d tau at fixed tau_factor, d/d tau_factor
    double* pi_out;                 // [cols][k]
    int* flat_out;                  // [cols]
};

// G lanes per branch, R states per lane (state g + G r of lane g: the G lanes of a unit read G consecutive doubles per load);
// 64 / G branches per wavefront, four wavefronts.  grid (piece, column).
// Every load is issued whatever the mask, the tip flag or the id say (a clamped address, a select afterwards), as exp_weight
// does: the loads of a step are independent of each other and overlap.
template <int G, int R>
__global__ void __launch_bounds__(256) gradient_f81_kernel(PmlGradArgs A) {
    constexpr int U = 64 / G, UNITS = 4 * U, ROW = G * R + 3;
    __shared__ double red[UNITS * ROW];
    const int k = A.k, ks = A.ks;
    const int lane = threadIdx.x & 63, g = lane % G;
    const int unit = (threadIdx.x >> 6) * U + lane / G;
    const int col = A.col0 + blockIdx.y;
    const size_t colN = (size_t)col * A.N;
    const double mu = A.mu[col], tau = A.tau[col], scale = A.tauf[col] * A.sf[col];
    double pi[R], acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int b = g + G * r;
        pi[r] = b < k ? A.pi[(size_t)col * ks + b] : 0.0;
        acc[r] = 0.0;
    }
    double T0 = 0.0, T1 = 0.0, n_flat = 0.0;
    const int i0 = blockIdx.x * A.piece, i1 = min(A.N, i0 + A.piece);
    for (int base = i0; base < i1; base += UNITS) {   // (the same trip count in every unit: the lane exchanges below are convergent)
        const int i = min(base + unit, i1 - 1);
        const bool inside = base + unit < i1;
        const int n = A.new_of_old ? A.new_of_old[i] : i;
        const int p = A.parent[n];
        const int pp = max(p, 0);
        const bool tip = A.n_children[n] == 0;
        const size_t row = colN + n;
        const double e = A.E[row];
        const double tt = (A.dist[n] + tau) * scale;   // (the transform of f81_prep_kernel)
        double v[R], q[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int b = g + G * r, bb = min(b, k - 1);
            const u64 m = A.masks[row * A.W + (bb >> 6)];
            const double x = A.bu[row * ks + bb];
            const double y = A.post[(colN + pp) * ks + bb];
            const bool allowed = b < k && ((m >> (bb & 63)) & 1ull);
            v[r] = allowed ? (tip ? 1.0 : x) : 0.0;
            q[r] = b < k ? y : 0.0;
        }
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) s += pi[r] * v[r];
        s = group_sum<G>(s);
        const double rest = (1.0 - e) * s;
        double a = 0.0, bsum = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double m = rest + e * v[r];
            const double f = (q[r] > 0.0 && m > 0.0) ? q[r] / m : 0.0;
            a += f;
            bsum += f * v[r];
        }
        a = group_sum<G>(a);
        bsum = group_sum<G>(bsum);
        const bool root = inside && p < 0;
        const bool flat = e == 1.0;
        const bool branch = inside && p >= 0 && !flat;
        const double h = branch ? -mu * e * (bsum - s * a) : 0.0;
        T0 += h;
        T1 += h * tt;
        n_flat += (inside && p >= 0 && flat) ? 1.0 : 0.0;
        const double c = branch ? -expm1(-mu * tt) * a : ((root && s > 0.0) ? 1.0 / s : 0.0);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] += c * v[r];
    }
    // the units' sums in unit order (every lane of a unit holds the unit's T0, T1 and count)
    double* mine = red + unit * ROW;
    if (g == 0) {
        mine[0] = T0;
        mine[1] = T1;
        mine[2] = n_flat;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) mine[3 + g + G * r] = acc[r];
    __syncthreads();
    double* out = A.partial + ((size_t)blockIdx.y * A.n_pieces + blockIdx.x) * (k + 3);
    for (int t = threadIdx.x; t < k + 3; t += 256) {
        double sum = 0.0;
        for (int j = 0; j < UNITS; ++j) sum += red[j * ROW + t];
        out[t] = sum;
    }
}

// The pieces' partials in piece order, and the natural derivatives from them.  grid (column); thread t < k + 3 owns one sum.
static __global__ void __launch_bounds__(256) gradient_reduce_kernel(PmlGradArgs A) {
    __shared__ double T[3];
    const int k = A.k;
    const int col = A.col0 + blockIdx.x;
    const double* part = A.partial + (size_t)blockIdx.x * A.n_pieces * (k + 3);
    double sums[3];   // entries t, t + 256, t + 512 of the k + 3 <= 515
#pragma unroll
    for (int h = 0; h < 3; ++h) {
        const int t = threadIdx.x + 256 * h;
        double s = 0.0;
        if (t < k + 3)
            for (int j = 0; j < A.n_pieces; ++j) s += part[(size_t)j * (k + 3) + t];
        sums[h] = s;
    }
    if (threadIdx.x < 3) T[threadIdx.x] = sums[0];
    __syncthreads();
    const double mu = A.mu[col], sf = A.sf[col], tf = A.tauf[col];
    if (threadIdx.x == 0) {
        A.rates_out[(size_t)blockIdx.x * 3 + 0] = T[1] / sf;
        A.rates_out[(size_t)blockIdx.x * 3 + 1] = T[0] * tf * sf;
        A.rates_out[(size_t)blockIdx.x * 3 + 2] = T[1] / tf;
        A.flat_out[blockIdx.x] = (int)T[2];
    }
#pragma unroll
    for (int h = 0; h < 3; ++h) {
        const int m = threadIdx.x + 256 * h - 3;
        if (m >= 0 && m < k) A.pi_out[(size_t)blockIdx.x * k + m] = sums[h] + 2.0 * mu * A.pi[(size_t)col * A.ks + m] * T[1];
    }
}
