// Stand-alone check of csrc/wset_plan.h (the bookkeeping of the working-set lasso: S, pos, eviction and compaction order,
// which rows of Gs are owed): compiled by the host compiler with -fsanitize=address,undefined and run by
// tests/test_wstep_ws_host.py.  Add / evict / compact sequences are replayed against a dense model - a set of columns, a
// full "Gram matrix" T[i][j] = f(i, j) of all columns - so that a slot that points at the wrong column, a stale pos or
// a compaction that moves in the wrong order is a mismatch or an out-of-bounds access here.
#include "../admm-for-rank-based-loss_amd/csrc/wset_plan.h"

#include <cstdio>
#include <set>
#include <vector>

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                              \
        }                                                         \
    } while (0)

static double T(int i, int j) { return (double)((i + 1) * 7919 % 1009) * (double)((j + 1) * 7919 % 1009) + (i == j ? 1.0 : 0.0); }

struct Model {
    WsetPlan p;
    int stride;
    std::vector<double> Gs;   // stride x stride, as the device holds it
    std::set<int> in;
    Model(long long ld, int cap, int stride_) : stride(stride_), Gs((size_t)stride_ * stride_, 0.0) { p.reset(ld, cap); }
    // what k_ws_gram_rows does with the rows add() says are owed: rows first .., their mirror columns below first
    bool add(const std::vector<int>& cols, bool fixed = false) {
        const int first = p.add(cols.data(), (int)cols.size(), fixed);
        if (first < 0) return false;
        for (int a = first; a < p.size(); ++a) {
            for (int b = 0; b < p.size(); ++b) Gs[(size_t)a * stride + b] = T(p.S[(size_t)a], p.S[(size_t)b]);
            for (int b = 0; b < first; ++b) Gs[(size_t)b * stride + a] = T(p.S[(size_t)b], p.S[(size_t)a]);
        }
        for (int c : cols) in.insert(c);
        return true;
    }
    int evict(const std::vector<double>& wS) {
        std::vector<int> keep;
        const std::vector<int> oldS = p.S;
        const std::vector<char> oldF = p.fixed;
        const int gone = p.evict(wS.data(), keep);
        if (gone == 0) return 0;
        CHECK((int)keep.size() == p.size());
        for (size_t a = 0; a + 1 < keep.size(); ++a) CHECK(keep[a] < keep[a + 1]);
        for (size_t a = 0; a < keep.size(); ++a) CHECK(keep[a] >= (int)a && oldS[(size_t)keep[a]] == p.S[a]);
        for (size_t a = 0; a < oldS.size(); ++a) {
            const bool stays = wS[a] != 0.0 || oldF[a];
            CHECK(stays == p.has(oldS[a]));
            if (!stays) in.erase(oldS[a]);
        }
        std::vector<double> out((size_t)stride * stride, -1.0);
        wset_compact_host(Gs.data(), out.data(), stride, keep.data(), p.size());
        Gs.swap(out);
        return gone;
    }
    void verify(long long ld) {
        CHECK(p.size() <= p.cap && p.cap <= WS_CAP && p.size() == (int)in.size() && p.room() == p.cap - p.size());
        CHECK((long long)p.pos.size() == ld && p.fixed.size() == p.S.size());
        long long members = 0;
        for (long long j = 0; j < ld; ++j) {
            const int a = p.pos[(size_t)j];
            CHECK(a >= -1 && a < p.size());
            CHECK((a >= 0) == (in.count((int)j) == 1) && p.has(j) == (a >= 0));
            if (a >= 0) {
                CHECK(p.S[(size_t)a] == (int)j);
                ++members;
            }
        }
        CHECK(members == p.size() && !p.has(-1) && !p.has(ld));
        for (int a = 0; a < stride; ++a)
            for (int b = 0; b < stride; ++b) {
                const double want = (a < p.size() && b < p.size()) ? T(p.S[(size_t)a], p.S[(size_t)b]) : 0.0;
                CHECK(Gs[(size_t)a * stride + b] == want);   // unused slots: exactly zero
            }
    }
};

int main() {
    CHECK(WS_SELECT <= WS_CAP && WS_MAX_ROUNDS >= WS_CAP);
    {   // add, refuse, evict, add again at a small capacity (stride = cap: every index is checked by the sanitizer)
        const long long ld = 40;
        Model m(ld, 8, 8);
        m.verify(ld);
        CHECK(m.add({39}, true));                       // the free coordinate first
        CHECK(m.add({3, 17, 5}));
        m.verify(ld);
        CHECK(!m.add({17}) && !m.add({40}) && !m.add({-1}) && !m.add({6, 6}));   // in S already, outside, twice in the list
        m.verify(ld);
        CHECK(m.add({0, 1, 2, 4}) && m.p.room() == 0);
        CHECK(!m.add({7}));                             // full
        m.verify(ld);
        CHECK(m.evict({0.0, 1.5, 0.0, -2.0, 0.0, 0.0, 3.0, 0.0}) == 4);   // slot 0 is fixed: it stays with w = 0
        m.verify(ld);
        CHECK(m.p.S == std::vector<int>({39, 3, 5, 2}) && m.p.fixed[0] == 1 && m.p.fixed[1] == 0);
        CHECK(m.evict({0.0, 1.0, 1.0, 1.0}) == 0);
        CHECK(m.add({17, 7}));                          // an evicted column comes back into a new slot
        m.verify(ld);
        CHECK(m.evict({0.0, 0.0, 0.0, 0.0, 0.0, 0.0}) == 5 && m.p.size() == 1);
        m.verify(ld);
    }
    {   // filling to WS_CAP in batches of WS_SELECT, the last columns of a wide vector included; then a full eviction round
        const long long ld = 20004;
        Model m(ld, WS_CAP, WS_CAP);
        std::vector<int> cols;
        int next = (int)ld - 1;
        while (m.p.room() > 0) {
            cols.clear();
            for (int i = 0; i < WS_SELECT && (int)cols.size() < m.p.room(); ++i, next -= 19) cols.push_back(next);
            CHECK(m.add(cols));
        }
        CHECK(m.p.size() == WS_CAP && !m.add({0}));
        m.verify(ld);
        std::vector<double> wS((size_t)WS_CAP, 0.0);
        for (int a = 0; a < WS_CAP; a += 3) wS[(size_t)a] = 1.0 + a;
        CHECK(m.evict(wS) == WS_CAP - (WS_CAP + 2) / 3);
        m.verify(ld);
        CHECK(m.add({0, 1, 2}));
        m.verify(ld);
    }
    {   // capacities outside the range are clamped
        WsetPlan p;
        p.reset(8, 0);
        CHECK(p.cap == 1);
        p.reset(8, WS_CAP + 5);
        CHECK(p.cap == WS_CAP);
    }
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("wset_plan: ok\n");
    return 0;
}
