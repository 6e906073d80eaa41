// Table test of the user -> device index map of chains of 1..7 joints (ilqr_planner_amd/csrc/ilqr_dofmap.hpp): every kind, nb_deriv and
// dof, restated entry by entry.  Includes nothing but that header (built with g++ by tests/test_narrow_chain_cpu.py).
#include <cstdio>

#include "ilqr_dofmap.hpp"

using namespace ilqr;

static int failures = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond);     \
            std::printf(__VA_ARGS__);                                         \
            std::printf("\n");                                                \
            failures++;                                                       \
        }                                                                     \
    } while (0)

// the map and its inverse agree, and the device entries that no user index reaches are exactly the padding
static void check_inverse(const IndexMap& m, int kind, int nd, int dof, const char* what) {
    int hit[MAP_MAX] = {0};
    for (int i = 0; i < m.n_user; i++) {
        CHECK(m.dev[i] >= 0 && m.dev[i] < m.n_dev, "%s kind %d nd %d dof %d: dev[%d] = %d", what, kind, nd, dof, i, m.dev[i]);
        if (m.dev[i] >= 0 && m.dev[i] < MAP_MAX) {
            hit[m.dev[i]]++;
            CHECK(m.usr[m.dev[i]] == i, "%s kind %d nd %d dof %d: usr[dev[%d]] = %d", what, kind, nd, dof, i, m.usr[m.dev[i]]);
        }
    }
    for (int j = 0; j < MAP_MAX; j++) {
        CHECK(hit[j] <= 1, "%s: device entry %d reached twice", what, j);
        if (!hit[j]) CHECK(m.usr[j] == -1, "%s kind %d nd %d dof %d: padding %d has usr %d", what, kind, nd, dof, j, m.usr[j]);
        if (j >= m.n_dev) CHECK(!hit[j], "%s: entry %d beyond n_dev", what, j);
    }
}

int main() {
    for (int kind = 0; kind < 4; kind++)
        for (int nd = 1; nd <= 2; nd++)
            for (int dof = 1; dof <= 7; dof++) {
                DofMap m;
                CHECK(dof_map(kind, nd, dof, m), "kind %d nd %d dof %d refused", kind, nd, dof);
                const int tm = (kind == 1 || kind == 3) ? 1 : 0;
                CHECK(m.dof == dof && m.identity() == (dof == 7), "dof %d", dof);
                CHECK(m.x.n_user == nd * dof + tm && m.x.n_dev == nd * 7 + tm, "kind %d nd %d dof %d: n_x %d -> %d", kind, nd, dof, m.x.n_user, m.x.n_dev);
                CHECK(m.u.n_user == dof + tm && m.u.n_dev == 7 + tm, "kind %d nd %d dof %d: n_u %d -> %d", kind, nd, dof, m.u.n_user, m.u.n_dev);
                for (int i = 0; i < dof; i++) {
                    CHECK(m.x.dev[i] == i && m.u.dev[i] == i, "joint %d", i);
                    if (nd == 2) CHECK(m.x.dev[dof + i] == 7 + i, "kind %d dof %d: velocity %d -> %d", kind, dof, i, m.x.dev[dof + i]);
                }
                if (tm) {
                    CHECK(m.x.dev[nd * dof] == nd * 7, "kind %d nd %d dof %d: time state -> %d", kind, nd, dof, m.x.dev[nd * dof]);
                    CHECK(m.u.dev[dof] == 7, "kind %d dof %d: time control -> %d", kind, dof, m.u.dev[dof]);
                }
                check_inverse(m.x, kind, nd, dof, "x");
                check_inverse(m.u, kind, nd, dof, "u");
                if (dof == 7)
                    for (int i = 0; i < m.x.n_user; i++) CHECK(m.x.dev[i] == i && m.x.usr[i] == i, "7 joints: identity at %d", i);
                if ((kind == 0 || kind == 1) && nd == 1) {  // kp_joint targets: the state map on n_f = 7 + tm slots
                    const IndexMap t = joint_target_map(m, 7 + tm);
                    CHECK(t.n_user == 7 + tm && t.n_dev == 7 + tm, "target widths");
                    for (int j = 0; j < t.n_dev; j++) CHECK(t.usr[j] == m.x.usr[j], "kind %d dof %d: target slot %d", kind, dof, j);
                }
            }
    DofMap m;
    CHECK(!dof_map(0, 1, 0, m), "dof 0 accepted");
    CHECK(!dof_map(0, 1, 8, m), "dof 8 accepted");
    CHECK(!dof_map(4, 1, 6, m), "kind 4 accepted");
    CHECK(!dof_map(0, 3, 6, m), "nb_deriv 3 accepted");
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
