// Host test of the segment plan of pml_history_through_time (csrc/pml_time_segments.h): compiled with pml_time_segments.cpp,
// plain C++, no HIP, no GPU.  Prints "OK <cases> <segments>" or the first failure.  tests/test_time_segments_host.py runs it.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "pml_time_segments.h"

static int n_cases = 0;
static long long n_segments = 0;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAILED %s: %s -- ", name, #cond); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            std::exit(1);                                 \
        }                                                 \
    } while (0)

struct Forest {
    std::vector<int> parent;
    std::vector<double> time;
};

// n_trees roots at different times; a node hangs under an earlier node, every `zero_every`-th one with no extent
static Forest random_forest(int n, int n_trees, int zero_every, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> ext(0.01, 1.0);
    Forest f;
    for (int r = 0; r < n_trees; ++r) {
        f.parent.push_back(-1);
        f.time.push_back(1990.0 + 3.25 * r);
    }
    for (int i = n_trees; i < n; ++i) {
        const int p = (int)(rng() % (unsigned)i);
        f.parent.push_back(p);
        f.time.push_back(zero_every && i % zero_every == 0 ? f.time[p] : f.time[p] + ext(rng));
    }
    return f;
}

static bool near(double a, double b, double ulps) { return std::fabs(a - b) <= ulps * DBL_EPSILON * std::max(1.0, std::fabs(b)); }

static void check_plan(const char* name, const Forest& f, const std::vector<double>& T) {
    const int N = (int)f.parent.size(), M = (int)T.size() - 1;
    PmlTimeSegments plan;
    const std::string why = pml_plan_time_segments(f.parent.data(), f.time.data(), N, T.data(), M, plan);
    CHECK(why.empty(), "%s", why.c_str());
    ++n_cases;
    n_segments += plan.n_segments();
    CHECK(plan.M == M && (int)plan.bin_off.size() == M + 2 && plan.bin_off[0] == 0, "M %d", plan.M);
    CHECK(plan.bin_off[M + 1] == plan.n_segments() && (int)plan.starts.size() == plan.n_segments() &&
              (int)plan.frac.size() == 4 * plan.n_segments(),
          "sizes");
    CHECK(plan.n_interval_segments() == plan.bin_off[M], "interval segments");
    // the brute-force count, bins outside, nodes inside: which (bin, node) pairs hold a segment, which are flagged
    int at = 0;
    for (int m = 0; m <= M; ++m) {
        CHECK(plan.bin_off[m] == at, "bin %d begins at %d, not %d", m, plan.bin_off[m], at);
        for (int n = 0; n < N; ++n) {
            const int p = f.parent[n];
            if (p < 0) continue;
            const double tp = f.time[p], tn = f.time[n];
            bool has, flag;
            if (m == M) {
                has = flag = tp <= T[M] && T[M] < tn;
            } else if (tn == tp) {
                has = (T[m] <= tn && tn < T[m + 1]) || (m == M - 1 && tn == T[M]);
                flag = false;
            } else {
                has = std::min(T[m + 1], tn) > std::max(T[m], tp);
                flag = tp <= T[m] && T[m] < tn;
                CHECK(!flag || has, "a branch alive at boundary %d has no segment in bin %d (node %d)", m, m, n);
            }
            if (!has) continue;
            CHECK(at < plan.n_segments() && plan.node[at] == n, "bin %d: segment %d is node %d, expected %d", m, at,
                  at < plan.n_segments() ? plan.node[at] : -1, n);
            CHECK(plan.starts[at] == (flag ? 1 : 0), "bin %d node %d: flag %d", m, n, plan.starts[at]);
            const double s1 = plan.frac[4 * at], w = plan.frac[4 * at + 1], r = plan.frac[4 * at + 2], u = plan.frac[4 * at + 3];
            CHECK(s1 >= 0 && w >= 0 && r >= 0 && s1 <= 1 && w <= 1 && r <= 1, "bin %d node %d: %g %g %g", m, n, s1, w, r);
            CHECK(near(s1 + w + r, 1.0, 2), "bin %d node %d: s1 + w + r = %.17g", m, n, s1 + w + r);
            CHECK(near(u, w + r, 2), "bin %d node %d: u = %.17g, w + r = %.17g", m, n, u, w + r);
            if (m == M) CHECK(w == 0.0 && r == u, "point segment of node %d: w = %g", n, w);
            else if (tn == tp) CHECK(s1 == 0.0 && w == 1.0 && r == 0.0, "zero-extent node %d: %g %g %g", n, s1, w, r);
            else CHECK(w > 0.0, "bin %d node %d: an empty segment", m, n);
            ++at;
        }
    }
    CHECK(at == plan.n_segments(), "%d segments, brute force counts %d", plan.n_segments(), at);
    // per branch, the segments tile its covered part: the next s1 is the last s1 + w; the first begins where the bins do
    std::vector<double> reached(N, -1.0);
    std::vector<double> last_r(N, -1.0);
    for (int i = 0; i < plan.n_interval_segments(); ++i) {
        const int n = plan.node[i];
        const double s1 = plan.frac[4 * i], w = plan.frac[4 * i + 1];
        if (reached[n] >= 0.0) CHECK(near(s1, reached[n], 2), "node %d: a segment begins at %.17g, the last ended at %.17g", n, s1, reached[n]);
        else if (f.time[n] > f.time[f.parent[n]])
            CHECK(near(s1, std::max(0.0, (T[0] - f.time[f.parent[n]]) / (f.time[n] - f.time[f.parent[n]])), 2), "node %d: first s1 %.17g", n, s1);
        reached[n] = s1 + w;
        last_r[n] = plan.frac[4 * i + 2];
    }
    for (int n = 0; n < N; ++n)
        if (reached[n] >= 0.0 && f.time[n] > f.time[f.parent[n]]) {
            const double end = std::min(1.0, (T[M] - f.time[f.parent[n]]) / (f.time[n] - f.time[f.parent[n]]));
            CHECK(near(reached[n], end, 4), "node %d: covered to %.17g, expected %.17g", n, reached[n], end);
            CHECK(near(last_r[n], 1.0 - end, 4), "node %d: r of the last segment %.17g", n, last_r[n]);
        }
    // the pieces: none straddles two bins, none is empty or larger than asked, together they are the bins in order
    for (int piece : {1, 7, 256, 4096})
        for (int with_points = 0; with_points < 2; ++with_points) {
            const PmlTimePieces cut = pml_cut_time_pieces(plan, piece, with_points != 0);
            const int bins = M + with_points;
            CHECK((int)cut.bin_piece_off.size() == bins + 1 && cut.bin_piece_off[0] == 0 && cut.bin_piece_off[bins] == cut.n_pieces(), "piece tables");
            CHECK(cut.piece_off[0] == 0 && cut.piece_off[cut.n_pieces()] == plan.bin_off[bins], "pieces cover %d", cut.piece_off[cut.n_pieces()]);
            for (int m = 0; m < bins; ++m) {
                const int p0 = cut.bin_piece_off[m], p1 = cut.bin_piece_off[m + 1];
                CHECK(p1 - p0 == (plan.bin_off[m + 1] - plan.bin_off[m] + piece - 1) / piece, "bin %d: %d pieces", m, p1 - p0);
                for (int p = p0; p < p1; ++p) {
                    const int size = cut.piece_off[p + 1] - cut.piece_off[p];
                    CHECK(cut.piece_off[p] >= plan.bin_off[m] && cut.piece_off[p + 1] <= plan.bin_off[m + 1], "piece %d leaves bin %d", p, m);
                    CHECK(size >= 1 && size <= piece && (size == piece || p == p1 - 1), "piece %d of bin %d holds %d", p, m, size);
                }
            }
        }
}

static void check_refused(const char* name, const Forest& f, const std::vector<double>& T, int M, const char* word) {
    PmlTimeSegments plan;
    plan.M = -7;
    plan.node.assign(3, 42);
    const std::string why = pml_plan_time_segments(f.parent.data(), f.time.data(), (int)f.parent.size(), T.data(), M, plan);
    ++n_cases;
    CHECK(!why.empty(), "accepted");
    CHECK(why.find(word) != std::string::npos, "the reason '%s' does not say '%s'", why.c_str(), word);
    CHECK(plan.M == -7 && plan.node.size() == 3 && plan.node[1] == 42 && plan.bin_off.empty(), "a refused call left a plan");
}

int main() {
    const char* name = "setup";
    // roots at different times, zero-extent branches inside and outside the bins
    const Forest f = random_forest(400, 3, 7, 1);
    const double first = *std::min_element(f.time.begin(), f.time.end()), last = *std::max_element(f.time.begin(), f.time.end());
    CHECK(last > first + 3.0, "span");
    name = "bins off the nodes";
    check_plan(name, f, {first - 0.5, first + 0.7131, first + 1.9, first + 2.00017, last - 0.3333, last + 0.25});
    name = "a boundary on a node time";
    {
        std::vector<double> T = {first, f.time[57], f.time[211], f.time[212], last};
        std::sort(T.begin(), T.end());
        T.erase(std::unique(T.begin(), T.end()), T.end());
        CHECK(T.size() >= 3, "boundaries");
        check_plan(name, f, T);
    }
    name = "empty bins before the first root and after the last tip";
    check_plan(name, f, {first - 30.0, first - 20.0, first - 10.0, first + 1.0, last + 1.0, last + 2.0, last + 3.0});
    name = "part of the tree";
    check_plan(name, f, {first + 1.1, first + 1.6, first + 2.4});
    name = "one bin";
    check_plan(name, f, {first, last});
    name = "everything outside";
    check_plan(name, f, {last + 1.0, last + 2.0});
    {
        name = "200 bins inside one branch";
        Forest g;
        g.parent = {-1, 0, 0, 1};
        g.time = {0.0, 10.0, 3.0, 10.0};
        std::vector<double> T;
        for (int m = 0; m <= 200; ++m) T.push_back(2.0 + 0.03 * m);
        check_plan(name, g, T);
        name = "a sliver of 1e-12 of a branch";
        PmlTimeSegments plan;
        const std::vector<double> S = {-1.0, 1e-11, 10.0 - 1e-11, 11.0};
        check_plan(name, g, S);
        CHECK(pml_plan_time_segments(g.parent.data(), g.time.data(), 4, S.data(), 3, plan).empty(), "refused");
        // node 1 spans [0, 10]: its first segment is 1e-12 of it, its last one too, each with all its digits
        CHECK(plan.node[0] == 1 && near(plan.frac[1] * 1e12, 1.0, 4), "w of the first sliver %.17g", plan.frac[1]);
        bool found = false;
        for (int i = plan.bin_off[2]; i < plan.bin_off[3]; ++i)
            if (plan.node[i] == 1) {
                found = true;
                CHECK(std::fabs(plan.frac[4 * i + 1] - (10.0 - (10.0 - 1e-11)) / 10.0) == 0.0, "w of the last sliver %.17g", plan.frac[4 * i + 1]);
                CHECK(plan.frac[4 * i + 2] == 0.0, "r of the last sliver %.17g", plan.frac[4 * i + 2]);
            }
        CHECK(found, "node 1 has no segment in the last bin");
        name = "a zero-extent branch on the last boundary";
        check_plan(name, g, {0.0, 5.0, 10.0});
        CHECK(pml_plan_time_segments(g.parent.data(), g.time.data(), 4, std::vector<double>{0.0, 5.0, 10.0}.data(), 2, plan).empty(), "refused");
        CHECK(plan.node[plan.bin_off[2] - 1] == 3 && plan.bin_off[3] == plan.bin_off[2], "node 3 belongs to the last bin, no point at T_M");
    }
    for (unsigned seed = 2; seed < 12; ++seed) {
        name = "random";
        const Forest g = random_forest(50 + 37 * (int)seed, 1 + (int)(seed % 4), (int)(seed % 5), seed);
        std::mt19937 rng(seed);
        std::vector<double> T;
        for (int m = 0; m < 2 + (int)(seed * 7 % 23); ++m) T.push_back(1988.0 + 0.001 * (double)(rng() % 12000u));
        T.push_back(g.time[g.time.size() / 2]);
        std::sort(T.begin(), T.end());
        T.erase(std::unique(T.begin(), T.end()), T.end());
        if (T.size() >= 2) check_plan(name, g, T);
    }
    // refusals
    name = "refusals";
    const std::vector<double> T = {first, first + 1.0, last};
    Forest bad = f;
    bad.time[123] = bad.time[bad.parent[123]] - 0.25;
    check_refused(name, bad, T, 2, "node 123 is earlier than its parent");
    check_refused(name, f, {first, first + 1.0, first + 1.0}, 2, "boundary 2");
    check_refused(name, f, {first + 2.0, first + 1.0, last}, 2, "strictly ascending");
    check_refused(name, f, T, 0, "M = 0");
    check_refused(name, f, T, -1, "M = -1");
    check_refused(name, f, {first, NAN, last}, 2, "boundary 1 is not finite");
    check_refused(name, f, {first, first + 1.0, INFINITY}, 2, "boundary 2 is not finite");
    bad = f;
    bad.time[77] = NAN;
    check_refused(name, bad, T, 2, "node 77 is not finite");
    bad = f;
    bad.parent[9] = 100000;
    check_refused(name, bad, T, 2, "node 9");
    std::printf("OK %d %lld\n", n_cases, n_segments);
    return 0;
}
