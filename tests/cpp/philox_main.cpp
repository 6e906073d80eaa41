// The generator of the closed-loop noise (ilqr_planner_amd/csrc/ilqr_noise.hpp) on the host: the three published known-answer vectors of
// Philox4x32-10, then the map from a counter to its two normals against the values the NumPy restatement (tests/closed_loop_noise.py) wrote
// to the file given as argv[1] (lines of: seed instance sample step pair z0 z1), within 1e-14 max(1, |z|), then the per-step draw: rolled and
// unrolled forms agree bit for bit, an entry with sigma 0 and a pair with both sigmas 0 get nothing, the last normal of an odd n_x is dropped.
// Built plain and with -fsanitize=address,undefined by tests/test_philox_cpu.py.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "ilqr_noise.hpp"

using namespace ilqr;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main(int argc, char** argv) {
    const uint32_t kat[3][10] = {
        {0, 0, 0, 0, 0, 0, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
        {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
        {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
    for (const auto& v : kat) {
        uint32_t r[4];
        philox4x32_10(v[0], v[1], v[2], v[3], v[4], v[5], r);
        CHECK(std::memcmp(r, v + 6, sizeof r) == 0, "known answer: %08x %08x %08x %08x", r[0], r[1], r[2], r[3]);
    }
    // the uniforms stay inside (0, 1]: the smallest is 2^-54, the largest rounds to 1 (ln 1 = 0: a zero radius, no NaN)
    CHECK(noise_uniform(0, 0) == std::ldexp(1.0, -54), "smallest uniform");
    CHECK(noise_uniform(0xffffffffu, 0xffffffffu) <= 1.0 && noise_uniform(0xffffffffu, 0xffffffffu) > 0.999, "largest uniform");

    int n = 0;
    double worst = 0;
    if (argc > 1) {
        std::FILE* f = std::fopen(argv[1], "r");
        CHECK(f != nullptr, "cannot open %s", argv[1]);
        unsigned long long seed;
        unsigned b, s, k, j;
        double e0, e1;
        while (f && std::fscanf(f, "%llu %u %u %u %u %la %la", &seed, &b, &s, &k, &j, &e0, &e1) == 7) {
            double z0, z1;
            noise_pair(seed, b, s, k, j, z0, z1);
            const double d0 = std::fabs(z0 - e0) / std::fmax(1.0, std::fabs(e0)), d1 = std::fabs(z1 - e1) / std::fmax(1.0, std::fabs(e1));
            CHECK(d0 <= 1e-14 && d1 <= 1e-14, "normals of (%llu, %u, %u, %u, %u): %a %a, expected %a %a", seed, b, s, k, j, z0, z1, e0, e1);
            worst = std::fmax(worst, std::fmax(d0, d1));
            n++;
        }
        if (f) std::fclose(f);
        CHECK(n >= 5, "only %d counters read", n);
    }

    // the per-step draw on n_x = 15 (pair 7 half used) and the mapped n_x = 3 of a 3-joint chain (device entries 0, 1, 2 of 7)
    double sigma[15];
    for (int i = 0; i < 15; i++) sigma[i] = 1e-3 * (i + 1);
    sigma[1] = 0;               // half a pair
    sigma[4] = sigma[5] = 0;    // a pair that is not generated
    double a[15], r[15];
    for (int i = 0; i < 15; i++) a[i] = r[i] = -7.0;
    const unsigned on_a = noise_draw<15, false, false>(99, 3, 4, 5, sigma, 15, nullptr, a), on_r = noise_draw<15, false, true>(99, 3, 4, 5, sigma, 15, nullptr, r);
    CHECK(on_a == on_r && on_a == (0x7fffu & ~(1u << 1) & ~(3u << 4)), "entries drawn: %x %x", on_a, on_r);
    CHECK(std::memcmp(a, r, sizeof a) == 0, "rolled and unrolled draws differ");
    CHECK(a[1] == -7.0 && a[4] == -7.0 && a[5] == -7.0, "an entry with sigma 0 was written");
    for (int j = 0; j < 8; j++) {
        double z0, z1;
        noise_pair(99, 3, 4, 5, j, z0, z1);
        if (sigma[2 * j] != 0) CHECK(a[2 * j] == sigma[2 * j] * z0, "entry %d", 2 * j);
        if (2 * j + 1 < 15 && sigma[2 * j + 1] != 0) CHECK(a[2 * j + 1] == sigma[2 * j + 1] * z1, "entry %d", 2 * j + 1);
    }
    const int usr[7] = {0, 1, 2, -1, -1, -1, -1};
    double m[7];
    for (int i = 0; i < 7; i++) m[i] = -7.0;
    const double s3[15] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};   // entries behind the user's n_x are read by nothing
    const unsigned on_m = noise_draw<7, true, true>(99, 3, 4, 5, s3, 3, usr, m);
    double z0, z1, z2, z3;
    noise_pair(99, 3, 4, 5, 0, z0, z1);
    noise_pair(99, 3, 4, 5, 1, z2, z3);
    CHECK(on_m == 7u && m[0] == z0 && m[1] == z1 && m[2] == z2 && m[3] == -7.0 && m[6] == -7.0, "mapped draw: %x", on_m);

    std::printf("%d counters against the restatement, worst deviation %.3e max(1, |z|)\n", n, worst);
    std::printf(fails ? "FAILED\n" : "ok\n");
    return fails ? 1 : 0;
}
