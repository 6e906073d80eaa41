// The shared tables of the batch solvers (ilqr_planner_amd/csrc/ilqr_batch_tables.hpp) on the host.  Includes nothing but that header
// (built with g++ by tests/test_batch_tables_cpu.py).
//   no argument:  the exact properties of the tables, of the signature and of the sizes; prints "ok"
//   wide | narrow  nd n_u T dt Kw ld psi_file|- out_file n_kp kp_t... R_diag...:  builds the tables of one case and writes them as raw doubles
//                 (wide: wt V G Et PZ ZPZ h0inv; narrow: psip H0 wt wr pp) for the numerical check of the Python test
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ilqr_batch_tables.hpp"

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

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(double));
}
static bool all_zero(const double* p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (p[i] != 0.0) return false;
    return true;
}

// a full-rank overlapping basis: K Gaussian bumps over the horizon, one copy per control coordinate
static std::vector<double> bumps(int steps, int K, int nu) {
    std::vector<double> psi((size_t)steps * nu * K * nu, 0.0);
    for (int k = 0; k < steps; k++)
        for (int j = 0; j < K; j++) {
            const double x = (double)k / (steps > 1 ? steps - 1 : 1), c = (double)j / (K > 1 ? K - 1 : 1);
            const double v = std::exp(-(x - c) * (x - c) * K * K);
            for (int i = 0; i < nu; i++) psi[(size_t)(k * nu + i) * K * nu + j * nu + i] = v;
        }
    return psi;
}

struct Case {
    std::vector<int> kp_t;
    std::vector<double> R, psi;
    BatchTableIn in;
    Case(int nd, int nu, int T, double dt, std::vector<int> kp, int Kw, int ld, std::vector<double> p) : kp_t(std::move(kp)), R(nu), psi(std::move(p)) {
        for (int i = 0; i < nu; i++) R[i] = 1e-5 * (1 + i);
        in.nd = nd; in.n_x = nd * nu; in.n_u = nu; in.T = T; in.dt = dt; in.Kw = Kw; in.ld = ld;
        fix();
    }
    Case(const Case& o) : kp_t(o.kp_t), R(o.R), psi(o.psi), in(o.in) { fix(); }
    void fix() {
        in.n_kp = (int)kp_t.size(); in.kp_t = kp_t.data(); in.R_diag = R.data(); in.psi = psi.empty() ? nullptr : psi.data();
    }
};

static void check_identity(int nd) {
    const int nu = 7, T = 12, N = (T - 1) * nu;
    std::vector<double> eye((size_t)N * N, 0.0);
    for (int i = 0; i < N; i++) eye[(size_t)i * N + i] = 1.0;
    Case built(nd, nu, T, 0.01, {0, 5, 6, T - 1}, N, N, {}), given(nd, nu, T, 0.01, {0, 5, 6, T - 1}, N, N, eye);
    std::vector<double> wt0, wr0, wt1, wr1;
    sens_tables(built.in, wt0, wr0);
    sens_tables(given.in, wt1, wr1);
    CHECK(same_bits(wt0, wt1), "nd %d: Wt of an explicit identity differs from the built-in identity", nd);
    CHECK(same_bits(wr0, wr1), "nd %d: Wr / V of an explicit identity differs from the built-in identity", nd);
    // keypoint 0 sits on step 0: Wt_0 and the block of the step before it are zero, and so is its V
    const size_t tile = (size_t)built.in.n_x * N;
    CHECK(all_zero(wt0.data(), 2 * tile), "nd %d: Wt of a keypoint on step 0", nd);
    CHECK(all_zero(wr0.data(), tile), "nd %d: V of a keypoint on step 0", nd);
    CHECK(!all_zero(wt0.data() + 2 * tile, tile) && !all_zero(wr0.data() + tile, tile), "nd %d: Wt, V of a keypoint on step 5 are empty", nd);
    // a keypoint on step 1: the true sensitivity sees B PSI_0, the shifted one (block 0 of Su is zero) nothing
    Case one(nd, nu, T, 0.01, {1, T - 1}, N, N, {});
    sens_tables(one.in, wt0, wr0);
    CHECK(!all_zero(wt0.data(), tile), "nd %d: Wt_1 is empty", nd);
    CHECK(all_zero(wt0.data() + tile, tile), "nd %d: Wt_0 is not zero", nd);
    CHECK(all_zero(wr0.data(), tile), "nd %d: the shifted V of a keypoint on step 1 is not zero", nd);
}

static void check_narrow(int nd) {
    const int nu = 7, T = 12, K = 2, Kw = K * nu, ld = 16;
    Case c(nd, nu, T, 0.01, {1, T - 1}, Kw, ld, bumps(T - 1, K, nu));
    NarrowTables t;
    narrow_tables(c.in, t);
    const int nx = c.in.n_x, N = c.in.rows();
    CHECK((int)t.psip.size() == N * ld && (int)t.H0.size() == ld * ld && (int)t.pp.size() == ld * ld, "narrow sizes");
    CHECK((int)t.wt.size() == 2 * 2 * nx * ld && (int)t.wr.size() == 2 * nx * ld, "narrow sensitivity sizes");
    for (int q = Kw; q < ld; q++) {
        for (int k = 0; k < N; k++) CHECK(t.psip[(size_t)k * ld + q] == 0.0, "padded column %d of PSI", q);
        for (size_t r = 0; r < t.wt.size() / ld; r++) CHECK(t.wt[r * ld + q] == 0.0, "padded column %d of Wt", q);
        for (size_t r = 0; r < t.wr.size() / ld; r++) CHECK(t.wr[r * ld + q] == 0.0, "padded column %d of Wr", q);
        for (int r = 0; r < ld; r++) {
            CHECK(t.pp[(size_t)r * ld + q] == 0.0 && t.pp[(size_t)q * ld + r] == 0.0, "padding of PSI'PSI at %d, %d", r, q);
            CHECK(t.H0[(size_t)r * ld + q] == (r == q ? 1.0 : 0.0) && t.H0[(size_t)q * ld + r] == (r == q ? 1.0 : 0.0), "padding of H0 at %d, %d", r, q);
        }
    }
    CHECK(all_zero(t.wr.data(), (size_t)nx * ld), "nd %d: the shifted W of a keypoint on step 1 is not zero", nd);
    Case g(c);  // the general path wants no sensitivities
    g.in.sens = false;
    NarrowTables u;
    narrow_tables(g.in, u);
    CHECK(same_bits(t.psip, u.psip) && same_bits(t.H0, u.H0) && u.wt.empty() && u.wr.empty() && u.pp.empty(), "tables without sensitivities");
}

static void check_wide(int nd) {
    const int nu = 7, T = 12, K = 3, Kw = K * nu;
    Case c(nd, nu, T, 0.01, {0, 5, 6, T - 1}, Kw, Kw, bumps(T - 1, K, nu));
    WideTables t;
    CHECK(wide_tables(c.in, t), "nd %d: a full-rank basis is refused", nd);
    const int m = c.in.n_kp * c.in.n_x;
    CHECK((int)t.G.size() == m * m && (int)t.ZPZ.size() == m * m && (int)t.Et.size() == 2 * m * m && (int)t.PZ.size() == c.in.rows() * m &&
              (int)t.h0inv.size() == Kw * Kw, "wide sizes");
    bool sym = true, nonzero = false;
    for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) {
            if (std::memcmp(&t.G[(size_t)i * m + j], &t.G[(size_t)j * m + i], sizeof(double))) sym = false;
            if (t.G[(size_t)i * m + j] != 0.0) nonzero = true;
        }
    CHECK(sym && nonzero, "nd %d: G is not exactly symmetric (or empty)", nd);
    Case id(nd, nu, T, 0.01, {0, 5, 6, T - 1}, (T - 1) * nu, (T - 1) * nu, {});
    CHECK(wide_tables(id.in, t) && t.h0inv.empty(), "the identity basis forms a Kw x Kw matrix");
    Case bad(c);  // a zero column: PSI'R PSI is singular
    for (int k = 0; k < bad.in.rows(); k++) bad.psi[(size_t)k * Kw + 3] = 0.0;
    CHECK(!wide_tables(bad.in, t), "a rank-deficient basis is accepted");
}

static void check_signature() {
    const int nu = 7, T = 12, K = 3, Kw = K * nu;
    Case a(1, nu, T, 0.01, {0, 5, 6, T - 1}, Kw, Kw, bumps(T - 1, K, nu));
    BatchTableSig sig;
    CHECK(!sig.same(a.in), "an empty signature matches");
    sig.set(a.in);
    Case b(a);  // equal values in other arrays
    CHECK(sig.same(a.in) && sig.same(b.in), "equal inputs are not the same");
    { Case c(a); c.in.T = T + 1; c.psi = bumps(T, K, nu); c.fix(); CHECK(!sig.same(c.in), "T"); }
    { Case c(a); c.in.dt = 0.02; CHECK(!sig.same(c.in), "dt"); }
    { Case c(a); c.kp_t[1] = 4; CHECK(!sig.same(c.in), "kp_t"); }
    { Case c(a); c.kp_t.pop_back(); c.fix(); CHECK(!sig.same(c.in), "n_kp"); }
    { Case c(a); c.R[6] *= 2; CHECK(!sig.same(c.in), "R_diag"); }
    { Case c(a); c.in.Kw = c.in.ld = Kw - nu; c.psi = bumps(T - 1, K - 1, nu); c.fix(); CHECK(!sig.same(c.in), "Kw"); }
    { Case c(a); c.in.ld = Kw + 1; CHECK(!sig.same(c.in), "ld"); }
    { Case c(a); c.in.nd = 2; c.in.n_x = 2 * nu; CHECK(!sig.same(c.in), "nd"); }
    { Case c(a); c.in.sens = false; CHECK(!sig.same(c.in), "sens"); }
    { Case c(a); c.psi.back() = std::nextafter(c.psi.back(), 2.0); CHECK(!sig.same(c.in), "last entry of PSI"); }
    { Case c(a); c.psi[0] = -c.psi[0]; CHECK(!sig.same(c.in), "first entry of PSI"); }
    {
        Case id(1, nu, T, 0.01, {0, 5, 6, T - 1}, (T - 1) * nu, (T - 1) * nu, {});
        CHECK(!sig.same(id.in), "the identity matches a basis");
        BatchTableSig s2;
        s2.set(id.in);
        CHECK(s2.same(id.in) && !s2.same(a.in), "identity signature");
    }
    sig.clear();
    CHECK(!sig.same(a.in), "a cleared signature matches");

    BatchSizes s;
    s.layout = BatchSizes::WIDE_LTI; s.n_x = 7; s.n_kp = 2; s.rows = 77; s.cols = 21; s.Bp = 64; s.ident = false;
    BatchSizes e = s;
    CHECK(e == s && !(e != s), "equal sizes differ");
    CHECK(BatchSizes() != s, "no buffers match");
    { BatchSizes c = s; c.layout = BatchSizes::WIDE_TIME; CHECK(c != s, "layout"); }
    { BatchSizes c = s; c.n_x = 14; CHECK(c != s, "n_x"); }
    { BatchSizes c = s; c.n_kp = 3; CHECK(c != s, "n_kp"); }
    { BatchSizes c = s; c.rows = 84; CHECK(c != s, "rows"); }
    { BatchSizes c = s; c.cols = 28; CHECK(c != s, "cols"); }
    { BatchSizes c = s; c.Bp = 128; CHECK(c != s, "Bp"); }
    { BatchSizes c = s; c.ident = true; CHECK(c != s, "ident"); }
}

static void write(std::FILE* f, const std::vector<double>& v) {
    if (!v.empty() && std::fwrite(v.data(), sizeof(double), v.size(), f) != v.size()) std::exit(3);
}

static int dump(int argc, char** argv) {
    if (argc < 11) return 2;
    const bool wide = !std::strcmp(argv[1], "wide");
    int a = 2;
    const int nd = std::atoi(argv[a++]), nu = std::atoi(argv[a++]), T = std::atoi(argv[a++]);
    const double dt = std::atof(argv[a++]);
    const int Kw = std::atoi(argv[a++]), ld = std::atoi(argv[a++]);
    const std::string psi_file = argv[a++], out_file = argv[a++];
    const int nkp = std::atoi(argv[a++]);
    if (argc != a + nkp + nu) return 2;
    std::vector<int> kp;
    for (int i = 0; i < nkp; i++) kp.push_back(std::atoi(argv[a++]));
    std::vector<double> psi;
    if (psi_file != "-") {
        psi.resize((size_t)(T - 1) * nu * Kw);
        std::FILE* f = std::fopen(psi_file.c_str(), "rb");
        if (!f || std::fread(psi.data(), sizeof(double), psi.size(), f) != psi.size()) return 3;
        std::fclose(f);
    }
    Case c(nd, nu, T, dt, kp, Kw, ld, psi);
    for (int i = 0; i < nu; i++) c.R[i] = std::atof(argv[a++]);
    std::FILE* f = std::fopen(out_file.c_str(), "wb");
    if (!f) return 3;
    if (wide) {
        std::vector<double> wt, V;
        sens_tables(c.in, wt, V);
        WideTables t;
        if (!wide_tables(c.in, t)) return 4;
        write(f, wt); write(f, V); write(f, t.G); write(f, t.Et); write(f, t.PZ); write(f, t.ZPZ); write(f, t.h0inv);
    } else {
        NarrowTables t;
        narrow_tables(c.in, t);
        write(f, t.psip); write(f, t.H0); write(f, t.wt); write(f, t.wr); write(f, t.pp);
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) return dump(argc, argv);
    for (int nd = 1; nd <= 2; nd++) {
        check_identity(nd);
        check_narrow(nd);
        check_wide(nd);
    }
    check_signature();
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
