// Host test of the upper ends of the segments (csrc/pml_time_segments.h: pml_time_segment_ends), which
// pml_sample_histories_through_time places events with: compiled with pml_time_segments.cpp, plain C++, no HIP, no GPU.  Prints
// "OK <cases> <segments> <chained>" or the first failure.  tests/test_time_segments_s2_host.py runs it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "pml_time_segments.h"

static int n_cases = 0;
static long long n_segments = 0, n_chained = 0;

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

// the forests of time_segments_driver.cpp: n_trees roots at staggered times, every `zero_every`-th node with no extent
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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

struct Seen {
    bool chained = false, zero = false, leaves = false, before = false, on_node = false;
};

static Seen check_ends(const char* name, const Forest& f, const std::vector<double>& T) {
    const int N = (int)f.parent.size(), M = (int)T.size() - 1;
    PmlTimeSegments plan;
    const std::string why = pml_plan_time_segments(f.parent.data(), f.time.data(), N, T.data(), M, plan);
    CHECK(why.empty(), "%s", why.c_str());
    const PmlTimeSegments before = plan;
    const PmlTimeSegmentEnds e = pml_time_segment_ends(plan);
    ++n_cases;
    n_segments += plan.n_segments();
    CHECK(plan.node == before.node && plan.frac == before.frac && plan.starts == before.starts && plan.bin_off == before.bin_off,
          "the plan changed");
    CHECK((int)e.s2.size() == plan.n_segments() && (int)e.ends.size() == plan.n_segments(), "sizes");
    std::map<std::pair<int, int>, int> at;   // (bin, node) -> segment
    for (int m = 0; m <= M; ++m)
        for (int i = plan.bin_off[m]; i < plan.bin_off[m + 1]; ++i) at[{m, plan.node[i]}] = i;
    Seen seen;
    for (int m = 0; m <= M; ++m)
        for (int i = plan.bin_off[m]; i < plan.bin_off[m + 1]; ++i) {
            const int n = plan.node[i];
            const double tp = f.time[f.parent[n]], tn = f.time[n], h = tn - tp;
            const double s1 = plan.frac[4 * i], r = plan.frac[4 * i + 2];
            const auto next = m < M ? at.find({m + 1, n}) : at.end();
            CHECK(e.ends[i] == 0 || e.ends[i] == 1, "bin %d node %d: flag %d", m, n, e.ends[i]);
            if (next != at.end()) {
                // the branch goes on: the next segment's s1, bit for bit -- the quotient (T_{m+1} - time_p) / h itself
                CHECK(!e.ends[i], "bin %d node %d goes on but ends", m, n);
                CHECK(same_bits(e.s2[i], plan.frac[4 * (size_t)next->second]), "bin %d node %d: s2 %.17g, the next s1 %.17g", m, n,
                      e.s2[i], plan.frac[4 * (size_t)next->second]);
                CHECK(same_bits(e.s2[i], (T[m + 1] - tp) / h), "bin %d node %d: s2 %.17g is not (T - tp) / h", m, n, e.s2[i]);
                CHECK(tn > T[m + 1] && r > 0.0, "bin %d node %d goes on with r = %g", m, n, r);
                CHECK(e.s2[i] >= s1, "bin %d node %d: s2 %.17g below s1 %.17g", m, n, e.s2[i], s1);
                seen.chained = true;
                ++n_chained;
                if (m + 1 == M) seen.leaves = true;   // (its next is the point segment at T_M)
            } else {
                CHECK(e.ends[i] == 1 && e.s2[i] == 1.0, "bin %d node %d ends here: s2 %.17g flag %d", m, n, e.s2[i], e.ends[i]);
                if (m < M) CHECK(tn <= T[m + 1] && r == 0.0, "bin %d node %d ends in the bin with r = %g", m, n, r);
            }
            if (h == 0.0) {
                CHECK(e.ends[i] == 1 && e.s2[i] == 1.0 && s1 == 0.0, "zero-extent node %d: s2 %.17g", n, e.s2[i]);
                seen.zero = true;
            }
            if (m == M) CHECK(e.ends[i] == 1 && e.s2[i] == 1.0, "point segment of node %d: s2 %.17g", n, e.s2[i]);
            if (h > 0.0 && tp < T[0] && m == 0) seen.before = true;
            if (h > 0.0 && m < M && (tp == T[m] || tn == T[m + 1])) seen.on_node = true;
        }
    // per branch: the segments in bin order tile [first s1, 1 or the point] without gap or overlap, in bits
    std::vector<int> last(N, -1);
    for (int m = 0; m <= M; ++m)
        for (int i = plan.bin_off[m]; i < plan.bin_off[m + 1]; ++i) {
            const int n = plan.node[i];
            if (last[n] >= 0) {
                CHECK(!e.ends[last[n]] && same_bits(e.s2[last[n]], plan.frac[4 * i]), "node %d: a gap or an overlap before bin %d", n, m);
            }
            last[n] = i;
        }
    for (int n = 0; n < N; ++n)
        if (last[n] >= 0) CHECK(e.ends[last[n]] == 1, "node %d: its last segment does not end", n);
    return seen;
}

int main() {
    const char* name = "setup";
    const Forest f = random_forest(400, 3, 7, 1);   // several roots at staggered times, zero-extent branches
    const double first = *std::min_element(f.time.begin(), f.time.end()), last = *std::max_element(f.time.begin(), f.time.end());
    name = "bins off the nodes";
    Seen s = check_ends(name, f, {first - 0.5, first + 0.7131, first + 1.9, first + 2.00017, last - 0.3333, last + 0.25});
    CHECK(s.chained && s.zero, "the case has no branch over two bins or none without extent");
    name = "a boundary on a node time";
    {
        std::vector<double> T = {first, f.time[57], f.time[211], f.time[212], last};
        std::sort(T.begin(), T.end());
        T.erase(std::unique(T.begin(), T.end()), T.end());
        s = check_ends(name, f, T);
        CHECK(s.on_node && s.chained, "no branch begins or ends on a boundary");
    }
    name = "part of the tree: branches that start before the range and branches that leave it";
    s = check_ends(name, f, {first + 1.1, first + 1.6, first + 2.4});
    CHECK(s.before && s.leaves, "before %d leaves %d", (int)s.before, (int)s.leaves);
    name = "one bin";
    check_ends(name, f, {first, last});
    name = "one bin inside: every crossing branch ends at its point segment";
    s = check_ends(name, f, {first + 1.3, first + 1.4});
    CHECK(s.leaves && s.before, "no branch crosses the bin");
    name = "everything outside";
    check_ends(name, f, {last + 1.0, last + 2.0});
    {
        name = "200 bins inside one branch";
        Forest g;
        g.parent = {-1, 0, 0, 1};
        g.time = {0.0, 10.0, 3.0, 10.0};
        std::vector<double> T;
        for (int m = 0; m <= 200; ++m) T.push_back(2.0 + 0.03 * m);
        s = check_ends(name, g, T);
        CHECK(s.chained && s.leaves && s.before && s.zero == false, "200 bins");
        name = "a sliver of 1e-12 of a branch";
        check_ends(name, g, {-1.0, 1e-11, 10.0 - 1e-11, 11.0});
        name = "a zero-extent branch on the last boundary";
        s = check_ends(name, g, {0.0, 5.0, 10.0});
        CHECK(s.zero && s.on_node, "node 3 on T_M");
    }
    for (unsigned seed = 2; seed < 14; ++seed) {
        name = "random";
        const Forest g = random_forest(50 + 37 * (int)seed, 1 + (int)(seed % 4), (int)(seed % 5), seed);
        std::mt19937 rng(seed);
        std::vector<double> T;
        for (int m = 0; m < 2 + (int)(seed * 7 % 23); ++m) T.push_back(1988.0 + 0.001 * (double)(rng() % 12000u));
        T.push_back(g.time[g.time.size() / 2]);
        std::sort(T.begin(), T.end());
        T.erase(std::unique(T.begin(), T.end()), T.end());
        if (T.size() >= 2) check_ends(name, g, T);
    }
    std::printf("OK %d %lld %lld\n", n_cases, n_segments, n_chained);
    return 0;
}
