// lpips_check.cpp -- a g++ build of csrc/lpips_math.h, the text lpips.hip runs, held against answers that need no recall of
// any package: stand-alone (its own main; exit status 0 and a last line "ok" when every check holds).
//   g++ -O2 -std=c++17 -ffp-contract=off tests/hostcheck/lpips_check.cpp -o lpips_check && ./lpips_check
#include <stdio.h>

#include <vector>

#include "../../d3ga_amd/csrc/lpips_math.h"

using namespace d3ga;

static int fails = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        if (!(cond)) {                                           \
            printf("FAILED line %d: %s\n", __LINE__, #cond);     \
            ++fails;                                             \
        }                                                        \
    } while (0)

static uint32_t rng = 12345u;
static float urand() {      // [0, 1)
    rng = rng * 1664525u + 1013904223u;
    return (float)(rng >> 8) * (1.f / 16777216.f);
}

static double distance64(int C, const float *a, const float *b, const float *lin) {
    double sa = 0, sb = 0, d = 0;
    for (int c = 0; c < C; ++c) { sa += (double)a[c] * a[c]; sb += (double)b[c] * b[c]; }
    const double na = sqrt(sa) + 1e-10, nb = sqrt(sb) + 1e-10;
    for (int c = 0; c < C; ++c) {
        const double t = a[c] / na - b[c] / nb;
        d += lin[c] * t * t;
    }
    return d;
}

int main() {
    // the plan of VGG16: 13 convolutions, pools in front of 2, 4, 7, 10, taps behind 1, 3, 6, 9, 12, widths 64 .. 512
    int pools = 0, taps = 0;
    for (int i = 0; i < kLpConvs; ++i) { pools += lp_pool_before(i); taps += lp_is_tap(i); }
    CHECK(pools == 4 && taps == kLpTaps && kLpMinSide == 1 << pools);
    for (int i = 0; i + 1 < kLpConvs; ++i) CHECK(!lp_pool_before(i + 1) || lp_is_tap(i));      // every pool follows a tap
    CHECK(lp_is_tap(kLpConvs - 1));
    CHECK(lp_vgg16_width(0) == 64 && lp_vgg16_width(1) == 64 && lp_vgg16_width(2) == 128 && lp_vgg16_width(3) == 128 && lp_vgg16_width(4) == 256 &&
          lp_vgg16_width(6) == 256 && lp_vgg16_width(7) == 512 && lp_vgg16_width(12) == 512);

    // the scaling layer against the formula in double, both settings
    const double shift[3] = {-.030, -.088, -.188}, scale[3] = {.458, .448, .450};
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k <= 16; ++k) {
            const float x = (float)k / 16.f;
            CHECK(fabs(lp_input(x, c, 0) - (x - shift[c]) / scale[c]) <= 4e-7 * 3);
            CHECK(fabs(lp_input(x, c, 1) - (2.0 * x - 1.0 - shift[c]) / scale[c]) <= 4e-7 * 3);
        }

    // the lane groups of the kernel cover every C in the passes it unrolls, and never more lanes than a wavefront
    for (int C = 1; C <= kLpMaxC; ++C)
        for (int vec = 0; vec <= ((C & 3) == 0); ++vec) {
            const int s = lp_group_shift(C, vec);
            CHECK(s >= 0 && s <= 6);
            CHECK((1 << s) * (vec ? 4 * kLpPassesVec : kLpPassesScalar) >= C);
            CHECK(s == 6 || (1 << s) * (vec ? 4 : 1) >= C);                       // below a wavefront: one pass covers C
            CHECK(s == 0 || (1 << (s - 1)) * (vec ? 4 : 1) < C);                  // and the group is the smallest such
        }
    CHECK(lp_tap_blocks(1, 0) == 1 && lp_tap_blocks(256, 0) == 1 && lp_tap_blocks(257, 0) == 2 && lp_tap_blocks(306, 4) == 20);
    CHECK(lp_tap_blocks((int64_t)1080 * 1920, 4) == kLpPartials && lp_tap_blocks(INT32_MAX, 6) == kLpPartials);

    // first-principles answers of the distance
    const int widths[] = {1, 2, 3, 8, 20, 33, 64, 512};
    for (int C : widths) {
        std::vector<float> a(C), b(C), lin(C), z(C, 0.f), a2(C), b2(C);
        for (int c = 0; c < C; ++c) lin[c] = urand() * 0.2f;
        lin[C / 2] = -0.05f;                                                     // a negative weight is accepted
        for (int i = 0; i < C; i += (C > 8 ? C / 4 : 1))
            for (int j = 0; j < C; j += (C > 8 ? C / 3 : 1)) {
                std::vector<float> ei(C, 0.f), ej(C, 0.f);
                ei[i] = 1.f; ej[j] = 1.f;
                if (i != j) CHECK(lp_pixel_distance(C, ei.data(), ej.data(), lin.data()) == lin[i] + lin[j]);      // one-hot pair
                else CHECK(lp_pixel_distance(C, ei.data(), ej.data(), lin.data()) == 0.f);
                CHECK(lp_pixel_distance(C, z.data(), ej.data(), lin.data()) == lin[j]);                            // a zero side: no NaN
                CHECK(lp_pixel_distance(C, ej.data(), z.data(), lin.data()) == lin[j]);
            }
        CHECK(lp_pixel_distance(C, z.data(), z.data(), lin.data()) == 0.f);
        for (int trial = 0; trial < 8; ++trial) {
            for (int c = 0; c < C; ++c) { a[c] = 0.5f + urand() * 2.f; b[c] = 0.5f + urand() * 2.f; }
            CHECK(lp_pixel_distance(C, a.data(), a.data(), lin.data()) == 0.f);                                    // a == b: exactly zero
            const float d = lp_pixel_distance(C, a.data(), b.data(), lin.data());
            const double d64 = distance64(C, a.data(), b.data(), lin.data());
            double mag = 0;                                                      // sum of |terms|: the scale of the rounding
            {
                double sa = 0, sb = 0;
                for (int c = 0; c < C; ++c) { sa += (double)a[c] * a[c]; sb += (double)b[c] * b[c]; }
                for (int c = 0; c < C; ++c) { const double t = a[c] / sqrt(sa) - b[c] / sqrt(sb); mag += fabs(lin[c]) * t * t; }
            }
            // float32 against double: a term passes through at most C + 8 roundings of relative size 2^-24 (two sums of C, a
            // root, two quotients, the products), and the difference of two unit-vector components below 1 carries an
            // absolute 2^-23 whatever it cancels to: (C + 8) 2^-21 (sum |terms| + mean |lin| / 8) covers both with room
            double lsum = 0;
            for (int c = 0; c < C; ++c) lsum += fabs(lin[c]);
            CHECK(fabs(d - d64) <= (C + 8) * 4.8e-7 * (mag + lsum / (8.0 * C)));
            // d(alpha a, beta b) = d(a, b): exact for powers of two (the norms here dwarf 1e-10), to rounding otherwise
            for (int c = 0; c < C; ++c) { a2[c] = 4.f * a[c]; b2[c] = 0.5f * b[c]; }
            CHECK(lp_pixel_distance(C, a2.data(), b2.data(), lin.data()) == d);
            for (int c = 0; c < C; ++c) { a2[c] = 3.7f * a[c]; b2[c] = 0.31f * b[c]; }
            CHECK(fabs(lp_pixel_distance(C, a2.data(), b2.data(), lin.data()) - d64) <= 2 * (C + 8) * 4.8e-7 * (mag + lsum / (8.0 * C)));
        }
    }
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("ok\n");
    return 0;
}
