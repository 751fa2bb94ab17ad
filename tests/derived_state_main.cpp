// Stand-alone print-out of csrc/derived_state.h: for every cause, set every flag, call the cause and list the flags that
// fell.  Compiled by the host compiler (with -fsanitize=address,undefined) and run by tests/test_derived_state_host.py,
// which holds the dependencies in its own words and compares cell by cell.
#include "../admm-for-rank-based-loss_amd/csrc/derived_state.h"

#include <cstdio>

struct Flag {
    const char* name;
    bool Derived::*at;
};
static const Flag FLAGS[] = {
    {"v_valid", &Derived::v_valid},         {"z_ready", &Derived::z_ready},
    {"p_valid", &Derived::p_valid},         {"p_pending", &Derived::p_pending},
    {"pred_valid", &Derived::pred_valid},   {"keys_ready", &Derived::keys_ready},
    {"s32_m_ready", &Derived::s32_m_ready}, {"s32_used", &Derived::s32_used},
    {"s32_q_done", &Derived::s32_q_done},   {"zb_used", &Derived::zb_used},
    {"zb_q_done", &Derived::zb_q_done},     {"zb_c_ready", &Derived::zb_c_ready},
    {"gram_local_done", &Derived::gram_local_done}, {"gram_ready", &Derived::gram_ready},
    {"eig_ok", &Derived::eig_ok},
};
struct Cause {
    const char* name;
    void (*fn)(Derived&);
};
static const Cause CAUSES[] = {
    {"data_changed", data_changed},       {"w_changed", w_changed},
    {"z_replaced", z_replaced},           {"lambda_changed", lambda_changed},
    {"rho_changed", rho_changed},         {"labels_changed", labels_changed},
    {"row_weights_changed", row_weights_changed}, {"gram_changed", gram_changed},
    {"drop_look_ahead", drop_look_ahead},
};

int main() {
    // every flag is a bool of the struct and nothing else is in it: a flag added to the header and not listed here shows
    static_assert(sizeof(Derived) == sizeof(FLAGS) / sizeof(FLAGS[0]) * sizeof(bool), "FLAGS does not list every flag of Derived");
    Derived fresh;
    for (const Flag& f : FLAGS)
        if (fresh.*f.at) std::printf("FAIL %s starts set\n", f.name);
    for (const Cause& c : CAUSES) {
        Derived s;
        for (const Flag& f : FLAGS) s.*f.at = true;
        c.fn(s);
        std::printf("%s:", c.name);
        for (const Flag& f : FLAGS)
            if (!(s.*f.at)) std::printf(" %s", f.name);
        std::printf("\n");
    }
    // the two produce sites of the Gram matrix
    Derived g;
    g.gram_ready = g.eig_ok = true;
    gram_formed(g);
    std::printf("gram_formed: local=%d ready=%d eig=%d\n", g.gram_local_done, g.gram_ready, g.eig_ok);
    gram_finished(g, true);
    std::printf("gram_finished: local=%d ready=%d eig=%d\n", g.gram_local_done, g.gram_ready, g.eig_ok);
    std::printf("derived_state: done\n");
    return 0;
}
