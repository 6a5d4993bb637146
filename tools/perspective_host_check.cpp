// Stand-alone check of the perspective launch's host twin (mj_host_perspective) for a sanitizer build of the library's host code:
// no GPU, no Python.  The arithmetic is the kernel's (csrc/affine.hip: transform_pixel, one function for both), so what the
// sanitizers see here is what every thread of k_perspective computes.  float-cast-overflow is the point: no double that is out of
// an int's range, infinite or NaN may ever be converted to an int — the inside test comes first.  The cases are those where such a
// double arises: a pole line inside the frame (also exactly on a column of pixel centres: x / 0), coefficients of 1e300 and
// 1e308 (overflow to infinity), a 0 / 0 pixel, and windows that reach far beyond the image — into exactly sized heap buffers
// (what AddressSanitizer watches), for the three filters and one and three components.  Every result is held to a plain
// restatement of the rule's inside test: a pixel that is outside must be fill, and the 0 / 0 column is fill.
//
//   make -C pyjpegdecoder_amd/csrc XFLAGS="-Xarch_host -fsanitize=address,undefined,float-cast-overflow" OUT=$PWD/build_san/libmijpeg_san.so OBJDIR=$PWD/build_san/obj
//   hipcc -std=c++17 -fsanitize=address,undefined,float-cast-overflow -Iinclude tools/perspective_host_check.cpp -Lbuild_san -lmijpeg_san -Wl,-rpath,$PWD/build_san -o build_san/perspective_host_check
//   UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 build_san/perspective_host_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "mijpeg.h"

struct Case {
    const char *name;
    int w, h;
    double c[8];
    int x0, y0, win_w, win_h;
};

int main() {
    int bad = 0, runs = 0;
    uint32_t seed = 2200;
    auto rnd = [&] { seed = seed * 1664525u + 1013904223u; return (uint8_t)(1 + (seed >> 24) % 250); };      // (never a fill byte)
    const double big = 1e300, top = 1e308;
    const std::vector<Case> cases = {
        {"identity", 48, 40, {1, 0, 0, 0, 1, 0, 0, 0}, 0, 0, 48, 40},
        {"keystone", 48, 40, {1.2, 0.3, -5, -0.2, 1.1, 4, 0.01, -0.008}, 0, 0, 48, 40},
        {"pole inside the frame", 48, 40, {1, 0, 0, 0, 1, 0, -0.05, 0}, 0, 0, 48, 40},
        {"pole on a column of pixel centres", 48, 40, {1, 0, 0, 0, 1, 0, -1 / 20.5, 0}, 0, 0, 48, 40},
        {"pole on a row of pixel centres", 21, 33, {1, 0, 0, 0, 1, 0, 0, -1 / 10.5}, 0, 0, 21, 33},
        {"source beyond the pole", 48, 40, {-1, 0, 0, 0, -1, 0, -1 / 10.25, 0}, 0, 0, 48, 40},
        {"1e300", 48, 40, {big, 0, 0, 0, big, 0, 0, 0}, 0, 0, 48, 40},
        {"1e300 everywhere", 21, 33, {big, -big, big, -big, big, -big, big, -big}, 0, 0, 21, 33},
        {"1e308: the sums overflow", 21, 33, {top, top, top, top, top, top, 0, 0}, 0, 0, 30, 40},
        {"1e308 in the denominator", 21, 33, {1, 0, 0, 0, 1, 0, -top, -top}, 0, 0, 21, 33},
        {"tiny denominator", 48, 40, {1, 0, 0, 0, 1, 0, -1 / 20.5 + 1e-17, 1e-300}, 0, 0, 48, 40},
        {"0 / 0 in column 0", 12, 10, {0, 0, 0, 0, 1, 0, -2, 0}, 0, 0, 12, 10},
        {"0 / 0 everywhere in x", 12, 10, {0, 0, 0, 0, 0, 0, -2, 0}, 0, 0, 1, 10},
        {"a window beyond the image", 48, 40, {1, 0, 0, 0, 1, 0, 0.002, 0.001}, 40, 30, 300, 200},
        {"a window at the coordinates' end", 21, 33, {0.0005, 0, 0, 0, 0.0005, 0, 0, 0}, 32000, 32000, 767, 767},
        {"a far window across a pole", 21, 33, {1, 0, 0, 0, 1, 0, -1 / 30000.5, 0}, 29990, 0, 40, 33},
        {"one pixel", 1, 1, {1, 0, 0, 0, 1, 0, 0.5, 0.5}, 0, 0, 5, 5},
    };
    for (const Case &k : cases)
        for (int ncomp : {1, 3})
            for (int filter : {MJ_AFFINE_NEAREST, MJ_AFFINE_BILINEAR, MJ_AFFINE_BICUBIC}) {
                std::vector<uint8_t> src((size_t)k.w * k.h * ncomp), out((size_t)k.win_w * k.win_h * ncomp, 77);
                for (uint8_t &v : src) v = rnd();
                const uint8_t fill[3] = {255, 254, 253};
                ++runs;
                if (mj_host_perspective(src.data(), k.w, k.h, ncomp, k.c, filter, fill, k.x0, k.y0, k.win_w, k.win_h, out.data()) != MJ_OK) {
                    ++bad; fprintf(stderr, "%s: refused\n", k.name);
                    continue;
                }
                // the rule's inside test, restated (volatile: every operation rounded on its own, whatever this file is compiled with)
                int wrong = 0;
                for (int y = 0; y < k.win_h; ++y)
                    for (int x = 0; x < k.win_w; ++x) {
                        volatile double xc = k.x0 + x + 0.5, yc = k.y0 + y + 0.5;
                        volatile double t0 = k.c[6] * xc, t1 = k.c[7] * yc, t2 = t0 + t1, d = t2 + 1;
                        volatile double n0 = k.c[0] * xc, n1 = k.c[1] * yc, n2 = n0 + n1, nx = n2 + k.c[2];
                        volatile double m0 = k.c[3] * xc, m1 = k.c[4] * yc, m2 = m0 + m1, ny = m2 + k.c[5];
                        volatile double xin = nx / d, yin = ny / d;
                        const bool inside = xin >= 0.0 && xin < k.w && yin >= 0.0 && yin < k.h;
                        const uint8_t *p = &out[((size_t)y * k.win_w + x) * ncomp];
                        bool is_fill = true;
                        for (int c = 0; c < ncomp; ++c) is_fill = is_fill && p[c] == fill[c];
                        // (nearest copies a source byte, which is never a fill byte; the interpolating filters may reach 255 by clamping)
                        if (!inside && !is_fill) ++wrong;
                        if (inside && is_fill && filter == MJ_AFFINE_NEAREST) ++wrong;
                    }
                if (wrong) { ++bad; fprintf(stderr, "%s, %d components, filter %d: %d pixels on the wrong side of the inside test\n", k.name, ncomp, filter, wrong); }
            }
    // refusals leave the buffer alone
    {
        std::vector<uint8_t> src(8 * 8 * 3, 9), out(1, 77);
        const double ident[8] = {1, 0, 0, 0, 1, 0, 0, 0}, with_nan[8] = {1, 0, nan(""), 0, 1, 0, 0, 0}, with_inf[8] = {1, 0, 0, 0, 1, 0, INFINITY, 0};
        if (mj_host_perspective(src.data(), 8, 8, 3, with_nan, MJ_AFFINE_BILINEAR, nullptr, 0, 0, 8, 8, out.data()) != MJ_ERR_INVALID) ++bad;
        if (mj_host_perspective(src.data(), 8, 8, 3, with_inf, MJ_AFFINE_BILINEAR, nullptr, 0, 0, 8, 8, out.data()) != MJ_ERR_INVALID) ++bad;
        if (mj_host_perspective(src.data(), 8, 8, 3, ident, 9, nullptr, 0, 0, 8, 8, out.data()) != MJ_ERR_INVALID) ++bad;
        if (mj_host_perspective(src.data(), 8, 8, 2, ident, MJ_AFFINE_NEAREST, nullptr, 0, 0, 8, 8, out.data()) != MJ_ERR_INVALID) ++bad;
        if (mj_host_perspective(src.data(), 8, 8, 3, ident, MJ_AFFINE_NEAREST, nullptr, 32760, 0, 8, 8, out.data()) != MJ_ERR_INVALID) ++bad;
        if (mj_host_perspective(src.data(), 32768, 1, 3, ident, MJ_AFFINE_NEAREST, nullptr, 0, 0, 1, 1, out.data()) != MJ_ERR_INVALID) ++bad;
        if (out[0] != 77) ++bad;
    }
    printf("perspective_host_check: %d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
