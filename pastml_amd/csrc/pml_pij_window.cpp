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

std::string pml_window_piece_runs(int n_ids, int piece, long long B, std::vector<PmlPieceRun>& out) {
    out.clear();
    if (piece < 1 || B < piece)
        return "a window of " + std::to_string(B) + " branches is below one piece of " + std::to_string(piece) + " ids";
    const int n_pieces = (n_ids + piece - 1) / piece;
    const int per = (int)std::min<long long>(B / piece, std::max(1, n_pieces));
    for (int p = 0; p < n_pieces; p += per) out.push_back(PmlPieceRun{p, std::min(n_pieces, p + per)});
    return "";
}

std::string pml_plan_sim_window(const PmlForest& f, int depth, long long B, PmlSimWindowPlan& out) {
    out = PmlSimWindowPlan();
    const int L = (int)f.td_offsets.size() - 1;
    if (B < 1) return "a window of " + std::to_string(B) + " branches";
    if (depth < 0 || depth > L) return "frontier depth " + std::to_string(depth) + " of " + std::to_string(L) + " levels";
    // nodes of the subtree below every node (a child's id is above its parent's: the depths are consecutive id ranges)
    std::vector<int> size((size_t)f.N, 1);
    for (int n = f.N - 1; n >= 0; --n)
        if (f.parent[n] >= 0) size[(size_t)f.parent[n]] += size[(size_t)n];
    int D = depth;
    for (; D < L; ++D) {
        int most = 0;
        for (int r = f.td_offsets[D]; r < f.td_offsets[D + 1]; ++r) most = std::max(most, size[(size_t)r]);
        if (most <= B) break;
    }
    out.depth = D;
    for (int d = 0; d < D; ++d) {
        const int a = f.td_offsets[d], b = f.td_offsets[d + 1];
        if (d == 0) {   // the roots draw from their own rows: one launch, nothing to build
            if (b > a) out.levels.push_back(PmlSimWindowRun{a, b - a, 0, 0});
            continue;
        }
        for (int first = a; first < b;) {
            const int count = (int)std::min<long long>(B, b - first);
            const int build_first = (int)out.order.size();
            for (int n = first; n < first + count; ++n) out.order.push_back(n);
            out.levels.push_back(PmlSimWindowRun{first, count, build_first, count});
            first += count;
        }
    }
    out.list_base = (int)out.order.size();
    out.sub_off.assign(1, 0);
    if (D >= L) return "";
    const int r0 = f.td_offsets[D], r1 = f.td_offsets[D + 1];
    std::vector<int> stack;
    for (int r = r0; r < r1; ++r) {
        stack.assign(1, r);
        while (!stack.empty()) {
            const int n = stack.back();
            stack.pop_back();
            out.order.push_back(n);
            for (int j = f.n_children[n] - 1; j >= 0; --j) stack.push_back(f.first_child[n] + j);
        }
        out.sub_off.push_back((int)out.order.size() - out.list_base);
    }
    for (int s = 0; s < r1 - r0;) {
        int e = s + 1;   // (a subtree alone fits: the frontier was moved until it does)
        while (e < r1 - r0 && (long long)out.sub_off[(size_t)e + 1] - out.sub_off[(size_t)s] <= B) ++e;
        out.groups.push_back(PmlSimWindowRun{s, e - s, out.list_base + out.sub_off[(size_t)s], out.sub_off[(size_t)e] - out.sub_off[(size_t)s]});
        s = e;
    }
    return "";
}
