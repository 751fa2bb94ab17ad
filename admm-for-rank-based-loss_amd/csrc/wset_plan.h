// wset_plan.h - the bookkeeping of the working-set lasso (wstep_ws.hip): which columns are in the working set S, in which
// slot, which rows of the sub-Gram matrix Gs are owed, and the order of an eviction's compaction.  Plain C++ (no HIP):
// run_wstep_ws keeps one of these on the host beside the device copies (S, pos), and tests/wset_plan_main.cpp replays add /
// evict / compact sequences against a dense model under the sanitizers.
//
//   S[a]   = the column in slot a, a < size() <= cap <= WS_CAP; slots fill in the order the columns arrive
//   pos[j] = the slot of column j, -1 outside S
//   fixed[a]: slot a holds a free coordinate (l1_j = 0, the unpenalised intercept): never evicted
// add() appends and returns the first new slot: the rows first .. size() - 1 of Gs are owed (k_ws_gram_rows forms them,
// and their mirror columns).  evict() drops the slots whose coefficient is zero and that are not fixed; the kept slots
// move down in ascending order of their old slot, keep[a'] = old slot of new slot a', and Gs'[a'][b'] =
// Gs[keep[a']][keep[b']] (k_ws_compact), everything from the new size on zero.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

constexpr int WS_CAP = 1024;      // slots at most: Gs is WS_CAP x WS_CAP doubles, 8 MB
constexpr int WS_SELECT = 64;     // columns one scan adds at most
constexpr int WS_MAX_ROUNDS = WS_CAP + 64;   // a round adds a column or ends the loop: S fills before the rounds run out

struct WsetPlan {
    int cap = WS_CAP;
    std::vector<int> S, pos;
    std::vector<char> fixed;

    void reset(int64_t ld, int cap_) {
        cap = cap_ < 1 ? 1 : cap_ > WS_CAP ? WS_CAP : cap_;
        S.clear();
        fixed.clear();
        pos.assign((std::size_t)ld, -1);
    }
    int size() const { return (int)S.size(); }
    int room() const { return cap - size(); }
    bool has(int64_t j) const { return j >= 0 && j < (int64_t)pos.size() && pos[(std::size_t)j] >= 0; }
    // appends the n columns (distinct, none of them in S, n <= room()); returns the first new slot, -1 when refused
    int add(const int* cols, int n, bool is_fixed = false) {
        if (n < 0 || n > room()) return -1;
        for (int i = 0; i < n; ++i)
            if (cols[i] < 0 || cols[i] >= (int)pos.size() || pos[(std::size_t)cols[i]] >= 0) return -1;
        const int first = size();
        for (int i = 0; i < n; ++i) {
            if (pos[(std::size_t)cols[i]] >= 0) {   // a column twice in the list: undo
                for (int k = first; k < size(); ++k) pos[(std::size_t)S[(std::size_t)k]] = -1;
                S.resize((std::size_t)first);
                fixed.resize((std::size_t)first);
                return -1;
            }
            pos[(std::size_t)cols[i]] = size();
            S.push_back(cols[i]);
            fixed.push_back(is_fixed ? 1 : 0);
        }
        return first;
    }
    // wS: the coefficients by slot (size() of them).  keep <- the old slots that stay, ascending; returns how many left
    int evict(const double* wS, std::vector<int>& keep) {
        keep.clear();
        const int m = size();
        for (int a = 0; a < m; ++a)
            if (wS[a] != 0.0 || fixed[(std::size_t)a]) keep.push_back(a);
        const int gone = m - (int)keep.size();
        if (gone == 0) return 0;
        for (int a = 0; a < m; ++a) pos[(std::size_t)S[(std::size_t)a]] = -1;
        std::vector<int> S2(keep.size());
        std::vector<char> f2(keep.size());
        for (std::size_t a = 0; a < keep.size(); ++a) {
            S2[a] = S[(std::size_t)keep[a]];
            f2[a] = fixed[(std::size_t)keep[a]];
            pos[(std::size_t)S2[a]] = (int)a;
        }
        S.swap(S2);
        fixed.swap(f2);
        return gone;
    }
};

// Gs' from Gs and keep, on the host (the replay of k_ws_compact; stride = WS_CAP on the device)
inline void wset_compact_host(const double* Gs, double* out, int stride, const int* keep, int m_new) {
    for (int a = 0; a < stride; ++a)
        for (int b = 0; b < stride; ++b)
            out[(std::size_t)a * stride + b] = (a < m_new && b < m_new) ? Gs[(std::size_t)keep[a] * stride + keep[b]] : 0.0;
}
