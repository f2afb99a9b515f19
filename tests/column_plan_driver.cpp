// Host-only check of the column layout's planner (pastml_amd/csrc/pml_columns.h).  argv[1]: tests/golden/column_plan.txt, the
// plans of the rules as they stood before the planner existed -- pml_plan_columns must reproduce every row exactly.  For every
// row the invariants no table expresses are checked as well: the lane groups hold the states, the padding, the parameter
// block's layout, that the lane shapes do not follow the number of columns; then the rejected inputs.
// Built and run by tests/test_column_plan_host.py; prints FAIL lines and exits 1, or one OK line.
#include "../pastml_amd/csrc/pml_columns.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

static int g_failures = 0;
static std::string g_case;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++g_failures <= 40) {                     \
                printf("FAIL [%s] ", g_case.c_str());     \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        }                                                 \
    } while (0)

static PmlTune no_tunables() {
    PmlTune t;   // (reads the environment: cleared)
    for (int i = 0; i < T_COUNT; ++i) t.has[i] = false, t.val[i] = 0;
    return t;
}

// level table of the fused bottom-up lists from "57x64" or "6x128+2x129": runs of count x units
static std::vector<int> offsets_of(const std::string& spec) {
    std::vector<int> off(1, 0);
    std::stringstream runs(spec);
    std::string run;
    while (std::getline(runs, run, '+')) {
        int n = 0, units = 0;
        if (sscanf(run.c_str(), "%dx%d", &n, &units) != 2) return {};
        for (int i = 0; i < n; ++i) off.push_back(off.back() + units);
    }
    return off;
}

static bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// the lane shapes and flags: everything but C, the block, thin_units and levels_fit_workgroup
static bool same_shapes(const PmlColumnPlan& a, const PmlColumnPlan& b) {
    return a.k == b.k && a.ks == b.ks && a.W == b.W && a.G == b.G && a.R == b.R && a.Gf == b.Gf && a.Rf == b.Rf && a.Gt == b.Gt &&
           a.Rt == b.Rt && a.bu_wide_lanes == b.bu_wide_lanes && a.level_lists_sorted == b.level_lists_sorted;
}

static bool same_plan(const PmlColumnPlan& a, const PmlColumnPlan& b) {
    const PmlParamBlock &x = a.params, &y = b.params;
    return same_shapes(a, b) && a.C == b.C && a.levels_fit_workgroup == b.levels_fit_workgroup && a.thin_units == b.thin_units &&
           x.pi == y.pi && x.sf == y.sf && x.tau == y.tau && x.tauf == y.tauf && x.mu == y.mu && x.kappa == y.kappa &&
           x.active == y.active && x.keep_tips == y.keep_tips && x.count == y.count;
}

static void check_invariants(const PmlColumnPlan& p, int n_cols, int k) {
    CHECK(p.C == n_cols && p.k == k, "C = %d k = %d", p.C, p.k);
    const int groups[3][2] = {{p.G, p.R}, {p.Gf, p.Rf}, {p.Gt, p.Rt}};
    for (const auto& g : groups) CHECK(is_pow2(g[0]) && g[0] * g[1] >= k, "lane group %d x %d for k = %d", g[0], g[1], k);
    CHECK(p.ks >= k && (k < 2 || p.ks % 2 == 0) && p.ks % p.R == 0, "ks = %d for k = %d, R = %d", p.ks, k, p.R);
    CHECK(p.W == (k + 63) / 64, "W = %d for k = %d", p.W, k);
    CHECK(p.bu_shape().g == (p.bu_wide_lanes ? 8 : p.Gf) && p.bu_shape().r == (p.bu_wide_lanes ? 8 : p.Rf), "bu_shape %d x %d",
          p.bu_shape().g, p.bu_shape().r);
    CHECK(p.td_shape().g == p.Gt && p.td_shape().r == p.Rt, "td_shape %d x %d", p.td_shape().g, p.td_shape().r);
    CHECK(p.shape(true).g == p.bu_shape().g && p.shape(false).g == p.td_shape().g, "shape(bottom_up)");
    // the block: pi [C][ks], then sf, tau, tauf, mu, kappa, active [C] each, then the keep-tips word, nothing else
    const PmlParamBlock& b = p.params;
    const size_t C = (size_t)n_cols, begin[9] = {b.pi, b.sf, b.tau, b.tauf, b.mu, b.kappa, b.active, b.keep_tips, b.count};
    const size_t size[8] = {C * p.ks, C, C, C, C, C, C, 1};
    CHECK(b.pi == 0, "pi at %zu", b.pi);
    for (int i = 0; i < 8; ++i) CHECK(begin[i] + size[i] == begin[i + 1], "array %d of the block: [%zu, +%zu) then %zu", i, begin[i], size[i], begin[i + 1]);
    CHECK(b.count == C * (p.ks + 6) + 1, "count = %zu", b.count);
    double probe[4] = {0, 0, 0, 0};
    CHECK(PmlParamBlock::at(probe, 3) == probe + 3 && PmlParamBlock::at((double*)nullptr, 3) == nullptr, "PmlParamBlock::at");
}

static void check_table(const char* path) {
    std::ifstream in(path);
    CHECK(in.good(), "cannot read %s", path);
    std::string line;
    int rows = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        g_case = line;
        int k = 0, n_cols = 0, want[12];
        long long value = 0;
        char traits[8], tunable[32], levels[64];
        const int got = sscanf(line.c_str(), "%d %d %7s %31s %lld %63s : %d %d %d %d %d %d %d %d %d %d %d %d", &k, &n_cols, traits, tunable,
                               &value, levels, want, want + 1, want + 2, want + 3, want + 4, want + 5, want + 6, want + 7, want + 8, want + 9,
                               want + 10, want + 11);
        CHECK(got == 18 && strlen(traits) == 3, "malformed row");
        if (got != 18 || strlen(traits) != 3) continue;
        ++rows;
        PmlForest f;
        f.polytomies = traits[0] == '1';
        f.balanced_parts = traits[1] == '1';
        f.shape_ordered = traits[2] == '1';
        f.bu_offsets_f = offsets_of(levels);
        f.N = 1000;
        CHECK(!f.bu_offsets_f.empty(), "malformed level table");
        PmlTune tune = no_tunables();
        if (strcmp(tunable, "-") != 0) {
            int var = -1;
            for (int i = 0; i < T_COUNT; ++i)
                if (strcmp(tunable, kTunableName[i]) == 0) var = i;
            CHECK(var >= 0, "unknown tunable %s", tunable);
            if (var < 0) continue;
            tune.has[var] = true;
            tune.val[var] = value;
        }
        PmlColumnPlan p;
        const std::string why = pml_plan_columns(f, tune, n_cols, k, p);
        CHECK(why.empty(), "rejected: %s", why.c_str());
        if (!why.empty()) continue;
        const int have[12] = {p.ks, p.W, p.G, p.R, p.Gf, p.Rf, p.Gt, p.Rt, (int)p.bu_wide_lanes, (int)p.level_lists_sorted,
                              (int)p.levels_fit_workgroup, p.thin_units};
        static const char* const name[12] = {"ks", "W", "G", "R", "Gf", "Rf", "Gt", "Rt", "bu_wide_lanes", "level_lists_sorted",
                                             "levels_fit_workgroup", "thin_units"};
        for (int i = 0; i < 12; ++i) CHECK(have[i] == want[i], "%s = %d, the table has %d", name[i], have[i], want[i]);
        check_invariants(p, n_cols, k);
        // the lane shapes follow k and the forest, never the columns
        for (int other : {1, 32, 4096, 65535}) {
            PmlColumnPlan q;
            CHECK(pml_plan_columns(f, tune, other, k, q).empty() && same_shapes(p, q), "the shapes change from %d to %d columns", n_cols, other);
            check_invariants(q, other, k);
        }
    }
    g_case = "table";
    CHECK(rows >= 1000, "%d rows", rows);
}

// every rejected input gives its reason and leaves `out` as it was
static void check_rejections() {
    PmlForest f;
    f.bu_offsets_f = {0, 1};
    f.N = 1000;
    const PmlTune tune = no_tunables();
    PmlColumnPlan marked;
    CHECK(pml_plan_columns(f, tune, 7, 20, marked).empty(), "the marker plan");
    auto rejected = [&](const char* what, const PmlForest& forest, int n_cols, int k, const std::string& reason) {
        g_case = what;
        PmlColumnPlan out = marked;
        const std::string why = pml_plan_columns(forest, tune, n_cols, k, out);
        CHECK(why == reason, "reason \"%s\", expected \"%s\"", why.c_str(), reason.c_str());
        CHECK(same_plan(out, marked), "`out` was written");
    };
    rejected("n_cols 0", f, 0, 4, "n_cols must be in 1..65535");
    rejected("n_cols 65536", f, 65536, 4, "n_cols must be in 1..65535");
    rejected("k 0", f, 32, 0, "k must be positive");
    rejected("k 513", f, 32, 513, "k = 513 states; at most 512 are supported");
    // a column's slab is addressed with 32-bit element offsets: N * ks one short of 2^31 is the last that is planned
    PmlForest big = f;
    big.N = 1 << 29;   // x ks = 4
    rejected("N * ks = 2^31", big, 32, 4, "n_nodes * k = 2147483648 exceeds 2^31 elements per column");
    big.N = (1 << 29) - 1;
    g_case = "N * ks = 2^31 - 4";
    PmlColumnPlan p;
    CHECK(pml_plan_columns(big, tune, 32, 4, p).empty() && p.ks == 4, "rejected below 2^31");
    big.N = (int)((1ll << 31) / 66 + 1);   // k = 65: rows padded to 66
    rejected("N * ks past 2^31, padded rows", big, 1, 65,
             "n_nodes * k = " + std::to_string((size_t)big.N * 66) + " exceeds 2^31 elements per column");
    f.bu_offsets_f.clear();   // (a forest without stored nodes: no levels, no thin ends)
    g_case = "no stored nodes";
    CHECK(pml_plan_columns(f, tune, 32, 4, p).empty() && !p.levels_fit_workgroup && p.thin_units == 0, "a forest without levels");
}

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: column_plan_driver tests/golden/column_plan.txt\n");
        return 2;
    }
    check_table(argv[1]);
    check_rejections();
    if (g_failures) {
        printf("%d failures\n", g_failures);
        return 1;
    }
    printf("OK column plans\n");
    return 0;
}
