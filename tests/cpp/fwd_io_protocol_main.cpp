// A host model of the hand-off protocol of k_forward_reg's helper-wave form (ilqr_planner_amd/csrc/ilqr_kernels_wave.hip, template parameter IO): the
// four chain waves, the gain loader, the x | u loader and the storer as state machines whose waits are the formulas of ilqr_fwd_io_plan.hpp, the
// header the kernel includes.  Every LDS access of the kernel's loop is one action of the model (a flag is written in an action of its own, after the
// data it announces), and a scheduler interleaves the waves' actions: seeded random orders, random orders in which a wave runs until it blocks, and
// the adversarial ones -- each helper always last, all helpers last, each chain wave always last -- for every subset of dead chain waves and every
// T1 = T - 1 from 0 to 3 FIO_RING + 1.  A run passes if every wave ends, every step of every live chain wave was read by the storer, every read found
// the step it expected in its slot, and no slot was overwritten before its last reader had read it.  Host-only (g++); built and run by
// tests/test_fwd_io_protocol_cpu.py.
#include <climits>
#include <cstdio>

#include "ilqr_fwd_io_plan.hpp"

using namespace ilqr;

namespace {

constexpr int NW = 4, GL = 4, VL = 5, ST = 6, NWAVES = 7, R = FIO_RING, G = FIO_GROUP;

struct Sim {
    int T1 = 0;
    bool live[NW] = {true, true, true, true};
    // the flag words
    int loaded_g = 0, loaded_v = 0, produced[NW] = {0, 0, 0, 0}, stored = 0;
    // the step each slot holds (-1: none); the out ring per chain wave's part of the slot
    int gslot[R], vslot[R], oslot[R][NW];
    int picked[NW], vread[NW], oread[NW];  // the last step of which wave w read the gains / xbar | ubar, the storer read wave w's x(1) | u(1)
    int pc[NWAVES] = {0, 0, 0, 0, 0, 0, 0}, n[NWAVES] = {0, 0, 0, 0, 0, 0, 0}, k0[NW] = {0, 0, 0, 0}, jj[NW] = {0, 0, 0, 0};
    bool done[NWAVES] = {false, false, false, false, false, false, false};
    int errors = 0;
    const char* first_error = "";

    void init(int t1, unsigned dead_mask) {
        T1 = t1;
        for (int s = 0; s < R; s++) { gslot[s] = vslot[s] = -1; for (int w = 0; w < NW; w++) oslot[s][w] = -1; }
        for (int w = 0; w < NW; w++) { live[w] = !((dead_mask >> w) & 1u); done[w] = !live[w]; picked[w] = vread[w] = oread[w] = -1; }
    }
    void fail(const char* what) { if (!errors) first_error = what; errors++; }
    int min_live() const {
        int m = INT_MAX;
        for (int w = 0; w < NW; w++) if (live[w] && produced[w] < m) m = produced[w];
        return m;
    }
    // one action of wave i; false: the wave is blocked in a wait
    bool step(int i) {
        if (i < NW) return chain(i);
        if (i == ST) return storer();
        return loader(i);
    }
    bool chain(int w) {
        const int k = k0[w] + jj[w];
        switch (pc[w]) {
            case 0:
                if (loaded_g < fio_need_loaded_g(0, T1)) return false;
                pc[w] = 1; return true;
            case 1: if (T1 > 0) { if (gslot[fio_slot(0)] != 0) fail("first pick: slot does not hold step 0"); picked[w] = 0; } pc[w] = 2; return true;
            case 2: if (k0[w] >= T1) { done[w] = true; return true; }
                    if (loaded_g < fio_need_loaded_g(k0[w], T1)) return false;
                    pc[w] = 3; return true;
            case 3:
                if (loaded_v < fio_need_loaded_v(k0[w], T1)) return false;
                pc[w] = 4; return true;
            case 4:
                if (stored < fio_need_stored(k0[w])) return false;
                jj[w] = 0; pc[w] = 5; return true;
            case 5: if (k + 1 < T1) { if (gslot[fio_slot(k + 1)] != k + 1) fail("pick: slot does not hold the next step"); picked[w] = k + 1; } pc[w] = k < T1 ? 6 : 9; return true;
            case 6: if (vslot[fio_slot(k)] != k) fail("xbar | ubar: slot does not hold the step"); vread[w] = k; pc[w] = 7; return true;
            case 7: { const int was = oslot[fio_slot(k)][w];
                      if (was >= 0 && oread[w] < was) fail("out ring: slot overwritten before the storer read it");
                      oslot[fio_slot(k)][w] = k; pc[w] = 8; return true; }
            case 8: produced[w] = k + 1; pc[w] = 9; return true;
            default: if (++jj[w] < G) pc[w] = 5; else { k0[w] += G; jj[w] = 0; pc[w] = 2; } return true;
        }
    }
    bool loader(int i) {
        const bool gl = i == GL;
        const int s = fio_slot(n[i]);
        switch (pc[i]) {
            case 0: if (n[i] >= T1) { done[i] = true; return true; }
                    if (min_live() < fio_need_produced_load(n[i])) return false;
                    pc[i] = 1; return true;
            case 1: { const int was = gl ? gslot[s] : vslot[s];
                      for (int w = 0; w < NW; w++) if (live[w] && was >= 0 && (gl ? picked[w] : vread[w]) < was) fail(gl ? "gain ring: slot overwritten before a chain wave read it" : "in ring: slot overwritten before a chain wave read it");
                      (gl ? gslot[s] : vslot[s]) = n[i]; pc[i] = 2; return true; }
            default: (gl ? loaded_g : loaded_v) = n[i] + 1; n[i]++; pc[i] = 0; return true;
        }
    }
    bool storer() {
        const int s = fio_slot(n[ST]);
        switch (pc[ST]) {
            case 0: if (n[ST] >= T1) { done[ST] = true; return true; }
                    if (min_live() < fio_need_produced_store(n[ST])) return false;
                    pc[ST] = 1; return true;
            case 1: for (int w = 0; w < NW; w++) if (live[w]) { if (oslot[s][w] != n[ST]) fail("storer: slot does not hold the step"); oread[w] = n[ST]; }
                    pc[ST] = 2; return true;
            default: stored = n[ST] + 1; n[ST]++; pc[ST] = 0; return true;
        }
    }
    bool all_done() const { for (int i = 0; i < NWAVES; i++) if (!done[i]) return false; return true; }
};

unsigned rng_state = 1;
unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// mode 0: a random wave per action; 1: a random wave runs until it blocks; 2: the waves of `last` (a mask) act only when no other wave can
// returns 0 ok, 1 blocked forever, 2 a check failed
int run(int T1, unsigned dead, int mode, unsigned last, const char** what) {
    Sim s;
    s.init(T1, dead);
    long actions = 0;
    while (!s.all_done()) {
        int order[NWAVES], m = 0;
        for (int pass = 0; pass < 2; pass++)   // the waves of `last` behind the others
            for (int i = 0; i < NWAVES; i++) if (!s.done[i] && (((last >> i) & 1u) != 0u) == (pass == 1)) order[m++] = i;
        int first_last = 0;
        while (first_last < m && !((last >> order[first_last]) & 1u)) first_last++;
        for (int a = first_last - 1; a > 0; a--) { const int b = (int)(rnd() % (unsigned)(a + 1)); const int t = order[a]; order[a] = order[b]; order[b] = t; }
        for (int a = m - 1; a > first_last; a--) { const int b = first_last + (int)(rnd() % (unsigned)(a - first_last + 1)); const int t = order[a]; order[a] = order[b]; order[b] = t; }
        bool moved = false;
        for (int q = 0; q < m && !moved; q++) {
            const int i = order[q];
            if (!s.step(i)) continue;
            moved = true; actions++;
            if (mode == 1) while (!s.done[i] && s.step(i)) actions++;
        }
        if (!moved) { *what = "no wave can act"; return 1; }
        if (actions > 10000000L) { *what = "runaway"; return 1; }
    }
    if (s.stored != T1) s.fail("not every step was stored");
    for (int w = 0; w < NW; w++) if (s.live[w] && T1 > 0 && (s.oread[w] != T1 - 1 || s.produced[w] != T1)) s.fail("a live chain wave's last step was not stored");
    if (s.loaded_g != T1 || s.loaded_v != T1) s.fail("not every step was loaded");
    if (s.errors) { *what = s.first_error; return 2; }
    return 0;
}

}  // namespace

int main() {
    int fails = 0;
    long runs = 0;
    for (int T1 = 0; T1 <= 3 * R + 1; T1++) {
        for (unsigned dead = 0; dead < 16u; dead++) {
            auto one = [&](int mode, unsigned last, const char* name) {
                const char* what = "";
                const int rc = run(T1, dead, mode, last, &what);
                runs++;
                if (rc && fails++ < 20) std::printf("FAIL T1 = %d dead = 0x%x %s: %s\n", T1, dead, name, what);
            };
            for (int seed = 0; seed < 24; seed++) { rng_state = 977u * (unsigned)seed + 31u * (unsigned)T1 + dead + 1u; one(0, 0u, "random"); one(1, 0u, "random, run until blocked"); }
            one(2, 1u << GL, "gain loader last"); one(2, 1u << VL, "x | u loader last"); one(2, 1u << ST, "storer last");
            one(2, (1u << GL) | (1u << VL) | (1u << ST), "helpers last");
            one(2, 0xfu, "chain waves last");
            for (int w = 0; w < NW; w++) { one(2, 1u << w, "one chain wave last"); one(1, 1u << w, "one chain wave last, run until blocked"); }
        }
    }
    if (fails) { std::printf("%d failures in %ld runs\n", fails, runs); return 1; }
    std::printf("%ld runs, ring %d, group %d\nok\n", runs, R, G);
    return 0;
}
