// The windowed form of a sweep plan (pml_pij_window.h).
#include "pml_pij_window.h"

#include <algorithm>

int pml_window_max_fanout(const PmlForest& f) {
    int most = 0;
    for (int n = 0; n < f.N; ++n) most = std::max(most, f.n_children[n]);
    return most;
}

std::string pml_plan_pij_window(const std::vector<PmlLaunch>& plan, const PmlForest& f, const std::vector<int>& bu_order,
                                const std::vector<int>& td_parents, long long B, PmlWindowPlan& out) {
    out = PmlWindowPlan();
    const int fan = pml_window_max_fanout(f);
    if (B < fan || B < 1)
        return "a window of " + std::to_string(B) + " branches is below the largest fan-out of the forest, " + std::to_string(fan);
    out.slot.assign((size_t)f.N, -1);
    for (const PmlLaunch& r : plan) {
        const bool level = r.op == OP_LEVEL && (r.list == L_BU_PLAIN || r.list == L_TD_PLAIN);
        if (!level || r.count <= 0) {
            out.steps.push_back(PmlWindowStep{r, 0, 0});
            continue;
        }
        const std::vector<int>& nodes = r.list == L_BU_PLAIN ? bu_order : td_parents;
        if (r.first < 0 || (size_t)r.first + (size_t)r.count > nodes.size())
            return "level record " + std::to_string(r.first) + " + " + std::to_string(r.count) + " beyond its list of " +
                   std::to_string(nodes.size()) + " nodes";
        // runs of consecutive parents of the record, greedily: a run is closed where the next parent's children no longer fit
        int run_first = r.first;
        long long held = 0;
        auto close = [&](int end, bool last) {
            PmlLaunch piece = r;
            piece.first = run_first;
            piece.count = end - run_first;
            piece.signal = last && r.signal;   // (the completion word is raised once, by the record's last run)
            const int build_first = (int)out.branches.size();
            for (int q = run_first; q < end; ++q) {
                const int p = nodes[q];
                for (int j = 0; j < f.n_children[p]; ++j) {
                    const int ch = f.first_child[p] + j;
                    out.slot[ch] = (int)out.branches.size() - build_first;
                    out.branches.push_back(ch);
                }
            }
            const int built = (int)out.branches.size() - build_first;
            out.steps.push_back(PmlWindowStep{piece, build_first, built});
            out.runs += built > 0 ? 1 : 0;
            run_first = end;
            held = 0;
        };
        for (int q = r.first; q < r.first + r.count; ++q) {
            const int nc = f.n_children[nodes[q]];
            if (held + nc > B) close(q, false);
            held += nc;
        }
        close(r.first + r.count, true);
    }
    return "";
}
