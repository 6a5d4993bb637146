// Stand-alone check of the two-step resize's host twins (mj_host_reduce_factors, mj_host_reduce, mj_host_resize_table_boxed) for
// a sanitizer build of the library's host code: no GPU, no Python.  It runs the functions over the shapes of
// tests/test_reduce_host.py — every factor pair 1..12 x 1..12 with remainders 0, 1 and f - 1, a few large cells, both phases — into
// exactly sized heap buffers (what AddressSanitizer watches), and holds mj_host_reduce to a plain restatement of Pillow's rule.
//
//   make -C pyjpegdecoder_amd/csrc XFLAGS="-Xarch_host -fsanitize=address,undefined" OUT=$PWD/build_san/libmijpeg_san.so OBJDIR=$PWD/build_san/obj
//   hipcc -std=c++17 -fsanitize=address,undefined -Iinclude tools/reduce_host_check.cpp -Lbuild_san -lmijpeg_san -Wl,-rpath,$PWD/build_san -o build_san/reduce_host_check
//   build_san/reduce_host_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mijpeg.h"

static uint32_t multiplier(uint32_t n) {
    volatile float q = 4294967296.0f / (float)(256u * n);
    return (uint32_t)q;
}

// Image.reduce on the array flipped along the axes that have a phase, flipped back
static void reference(const std::vector<uint8_t> &src, int w, int h, int c, int fx, int fy, bool back_x, bool back_y, std::vector<uint8_t> &out) {
    const int ow = (w + fx - 1) / fx, oh = (h + fy - 1) / fy;
    out.assign((size_t)ow * oh * c, 0);
    for (int Y = 0; Y < oh; ++Y)
        for (int X = 0; X < ow; ++X)
            for (int k = 0; k < c; ++k) {
                const int x0 = X * fx, x1 = std::min(w, x0 + fx), y0 = Y * fy, y1 = std::min(h, y0 + fy);
                uint32_t sum = 0;
                for (int y = y0; y < y1; ++y)
                    for (int x = x0; x < x1; ++x) sum += src[((size_t)(back_y ? h - 1 - y : y) * w + (back_x ? w - 1 - x : x)) * c + k];
                const uint32_t n = (uint32_t)(x1 - x0) * (uint32_t)(y1 - y0);
                out[((size_t)(back_y ? oh - 1 - Y : Y) * ow + (back_x ? ow - 1 - X : X)) * c + k] = (uint8_t)(((sum + n / 2) * multiplier(n)) >> 24);
            }
}

int main() {
    int bad = 0, runs = 0;
    uint32_t seed = 12345;
    auto rnd = [&] { seed = seed * 1664525u + 1013904223u; return (uint8_t)(seed >> 24); };
    struct Case { int w, h, fx, fy; };
    std::vector<Case> cases;
    for (int fx = 1; fx <= 12; ++fx)
        for (int fy = 1; fy <= 12; ++fy)
            for (int r = 0; r < 3; ++r) cases.push_back({3 * fx + (r == 0 ? 0 : r == 1 ? 1 : fx - 1), 2 * fy + (r == 0 ? 0 : r == 1 ? 1 : fy - 1), fx, fy});
    for (const Case &c : {Case{300, 9, 291, 2}, Case{128, 64, 32, 16}, Case{70, 513, 3, 256}, Case{600, 3, 600, 3}, Case{257, 300, 256, 256}, Case{40, 40, 41, 50}})
        cases.push_back(c);
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case &k = cases[i];
        const int c = (i & 1) ? 3 : 1;
        std::vector<uint8_t> src((size_t)k.w * k.h * c), want;
        for (uint8_t &v : src) v = rnd();
        const int ow = (k.w + k.fx - 1) / k.fx, oh = (k.h + k.fy - 1) / k.fy;
        for (int ph = 0; ph < 4; ++ph) {
            const int px = (ph & 1) ? k.w % k.fx : 0, py = (ph & 2) ? k.h % k.fy : 0;
            std::vector<uint8_t> out((size_t)ow * oh * c);
            if (mj_host_reduce(src.data(), k.w, k.h, c, k.fx, k.fy, px, py, out.data()) != MJ_OK) { ++bad; continue; }
            reference(src, k.w, k.h, c, k.fx, k.fy, (ph & 1) != 0, (ph & 2) != 0, want);
            if (out != want) { ++bad; fprintf(stderr, "reduce %d x %d by %d x %d, phases %d %d: differs\n", k.w, k.h, k.fx, k.fy, px, py); }
            ++runs;
        }
    }
    // refusals leave the buffers alone
    {
        std::vector<uint8_t> src(10 * 7 * 3), out(1);
        if (mj_host_reduce(src.data(), 10, 7, 3, 300, 300, 0, 0, out.data()) != MJ_ERR_INVALID) ++bad;
        if (mj_host_reduce(src.data(), 10, 7, 3, 3, 2, 2, 0, out.data()) != MJ_ERR_INVALID) ++bad;
        if (mj_host_reduce(src.data(), 10, 7, 2, 3, 2, 0, 0, out.data()) != MJ_ERR_INVALID) ++bad;
    }
    // factors, then the boxed table of each axis the factors give, into exactly sized arrays
    const int sizes[][4] = {{1920, 1080, 224, 224}, {70, 50, 8, 7}, {128, 64, 4, 4}, {100, 36, 12, 18}, {37, 29, 5, 4}, {65535, 3, 2, 1}, {9, 9, 9, 9}, {5000, 4000, 3, 3}};
    const double gaps[] = {1.0, 1.5, 2.0, 3.0};
    for (const auto &s : sizes)
        for (double gap : gaps) {
            int32_t fx = 0, fy = 0;
            if (mj_host_reduce_factors(s[0], s[1], s[2], s[3], gap, &fx, &fy) != MJ_OK || fx < 1 || fy < 1) { ++bad; continue; }
            for (int axis = 0; axis < 2; ++axis) {
                const int size = s[axis], f = axis ? fy : fx, out_size = s[2 + axis], in_size = (size + f - 1) / f;
                for (int filter = MJ_FILTER_BILINEAR; filter <= MJ_FILTER_LANCZOS; ++filter) {
                    int32_t ks = 0;
                    if (mj_host_resize_table_boxed(filter, in_size, 0.0, (double)size / f, out_size, nullptr, nullptr, nullptr, 0, &ks) != MJ_OK || ks < 1) { ++bad; continue; }
                    std::vector<int32_t> xmin((size_t)out_size), count((size_t)out_size), taps((size_t)out_size * ks);
                    if (mj_host_resize_table_boxed(filter, in_size, 0.0, (double)size / f, out_size, xmin.data(), count.data(), taps.data(), ks, nullptr) != MJ_OK) { ++bad; continue; }
                    for (int j = 0; j < out_size; ++j)
                        if (xmin[j] < 0 || count[j] < 0 || count[j] > ks || xmin[j] + count[j] > in_size) { ++bad; break; }
                    ++runs;
                }
            }
        }
    int32_t ks = 0;
    if (mj_host_resize_table_boxed(MJ_FILTER_BOX, 40, 0.0, 40.5, 9, nullptr, nullptr, nullptr, 0, &ks) != MJ_ERR_INVALID) ++bad;
    if (mj_host_resize_table_boxed(MJ_FILTER_BOX, 40, 0.0, nan(""), 9, nullptr, nullptr, nullptr, 0, &ks) != MJ_ERR_INVALID) ++bad;
    printf("reduce_host_check: %d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
