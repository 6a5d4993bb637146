// Stand-alone check of the patchify launch's host twin (mj_host_patchify) for a sanitizer build of the library's host code: no GPU,
// no Python.  The job list and the address rule are the launch's own (csrc/patch_addr.h, one set of functions for both), so what
// AddressSanitizer and the undefined-behaviour sanitizer see here — every element read and written, in every layout and element
// size, on EXACTLY sized heap buffers — is the ranges the workgroups of k_patchify are handed.  The cases are those of
// tests/patch_cases.py: the grid of patch x merge on a 48 x 36 and a 45 x 33 canvas with five windows each (an odd origin, a single
// merge block, a single band, a single block column, one window twice), whole canvases, rows of 27, 196 and 588 bytes, both padded
// forms, Qwen's shape, and the many-jobs sources.  Every result is held to a plain restatement of the rule on (c, y, x) coordinates,
// and mj_host_patchify_count to the sum of the grids.
//
//   make -C pyjpegdecoder_amd/csrc XFLAGS="-Xarch_host -fsanitize=address,undefined" OUT=$PWD/build_san/libmijpeg_san.so OBJDIR=$PWD/build_san/obj
//   hipcc -std=c++17 -fsanitize=address,undefined -Iinclude tools/patch_host_check.cpp -Lbuild_san -lmijpeg_san -Wl,-rpath,$PWD/build_san -o build_san/patch_host_check
//   UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 build_san/patch_host_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mijpeg.h"

typedef std::vector<mj_patch_window> Windows;

// element offset of (c, y, x) inside one W x H slot
static size_t at(int layout, int W, int H, int C, int c, int y, int x) {
    switch (layout) {
        case MJ_LAYOUT_XMAJOR: return ((size_t)x * H + y) * C + c;
        case MJ_LAYOUT_ROWMAJOR: return ((size_t)y * W + x) * C + c;
        case MJ_LAYOUT_PLANAR_XMAJOR: return ((size_t)c * W + x) * H + y;
        default: return ((size_t)c * H + y) * W + x;
    }
}

struct Case {
    std::string name;
    int W, H, C, N;
    int P, m, t, order, length;
    Windows windows;        // empty: NULL, every source's whole canvas
    int only_dtype;         // -1: all four
};

// tests/patch_cases.py: five_windows
static Windows five(int W, int H, int u) {
    if (u > W || u > H) return {};
    const bool odd = u <= W - 5 && u <= H - 3;
    const int ox = odd ? 5 : 0, oy = odd ? 3 : 0;
    const mj_patch_window big{ox, oy, (W - ox) / u * u, (H - oy) / u * u};
    auto fx = [&](int x) { return x + u <= W ? x : 0; };
    auto fy = [&](int y) { return y + u <= H ? y : 0; };
    const int bx = fx(3), by = fy(1), cx = fx(2), cy = fy(0);
    return {big, mj_patch_window{fx(1), fy(2), u, u}, mj_patch_window{bx, by, (W - bx) / u * u, u}, mj_patch_window{cx, cy, u, (H - cy) / u * u}, big};
}

static int64_t tokens(const Case &cs, int k) {
    const mj_patch_window w = cs.windows.empty() ? mj_patch_window{0, 0, cs.W, cs.H} : cs.windows[(size_t)k];
    return (int64_t)(w.width / cs.P) * (w.height / cs.P);
}

static std::vector<Case> cases() {
    std::vector<Case> out;
    const int canvases[2][2] = {{48, 36}, {45, 33}}, patches[5] = {1, 2, 3, 14, 16}, forms[3][2] = {{1, MJ_PATCH_CHW}, {2, MJ_PATCH_CHW}, {1, MJ_PATCH_HWC}};
    int idx = 0;
    for (const auto &cv : canvases)
        for (int P : patches)
            for (int m = 1; m <= 3; ++m) {
                const Windows w = five(cv[0], cv[1], P * m);
                if (w.empty()) continue;
                out.push_back({"grid", cv[0], cv[1], (idx / 3 + idx) % 2 ? 3 : 1, 5, P, m, forms[idx % 3][0], forms[idx % 3][1], 0, w, -1});
                ++idx;
            }
    const int whole[6][5] = {{1, 1, 1, MJ_PATCH_CHW, 3}, {2, 2, 2, MJ_PATCH_CHW, 1}, {3, 1, 1, MJ_PATCH_HWC, 3}, {4, 3, 1, MJ_PATCH_CHW, 3}, {6, 2, 1, MJ_PATCH_HWC, 1},
                             {12, 1, 2, MJ_PATCH_CHW, 3}};
    for (const auto &w : whole) out.push_back({"whole", 48, 36, w[4], 5, w[0], w[1], w[2], w[3], 0, {}, -1});
    out.push_back({"whole_odd_canvas", 45, 33, 3, 5, 3, 1, 1, MJ_PATCH_HWC, 0, {}, -1});
    out.push_back({"none_among_windows", 48, 36, 3, 5, 2, 3, 2, MJ_PATCH_CHW, 0, {{0, 0, 48, 36}, {5, 3, 12, 6}, {0, 0, 48, 36}, {1, 1, 6, 30}, {42, 30, 6, 6}}, -1});
    const int rows[5][3] = {{3, 3, MJ_PATCH_CHW}, {3, 3, MJ_PATCH_HWC}, {14, 1, MJ_PATCH_CHW}, {14, 3, MJ_PATCH_CHW}, {14, 3, MJ_PATCH_HWC}};
    for (const auto &r : rows) out.push_back({"row_bytes", 45, 33, r[1], 5, r[0], 1, 1, r[2], 0, five(45, 33, r[0]), -1});
    const int padded[3][5] = {{2, 2, 1, MJ_PATCH_CHW, 3}, {3, 1, 1, MJ_PATCH_HWC, 3}, {14, 1, 2, MJ_PATCH_CHW, 1}};
    for (const auto &p : padded) {
        Case cs{"padded_exact", 45, 33, p[4], 5, p[0], p[1], p[2], p[3], 0, five(45, 33, p[0] * p[1]), -1};
        int64_t longest = 0;
        for (int k = 0; k < 5; ++k) longest = std::max(longest, tokens(cs, k));
        cs.length = (int)longest;
        out.push_back(cs);
        cs.name = "padded_long"; cs.length = (int)longest * 2 + 37;
        out.push_back(cs);
    }
    out.push_back({"padded_whole", 48, 36, 1, 5, 4, 3, 1, MJ_PATCH_CHW, 200, {}, -1});
    out.push_back({"qwen", 61, 90, 3, 5, 14, 2, 2, MJ_PATCH_CHW, 0, {{0, 0, 56, 84}, {5, 3, 56, 84}, {4, 6, 56, 56}, {1, 0, 28, 84}, {5, 3, 56, 84}}, -1});
    // many jobs, one source each
    out.push_back({"wide", 4201, 29, 3, 1, 14, 2, 1, MJ_PATCH_CHW, 0, {{1, 1, 4200, 28}}, 3});
    out.push_back({"tall", 29, 2801, 3, 1, 14, 2, 1, MJ_PATCH_CHW, 0, {{1, 1, 28, 2800}}, 3});
    out.push_back({"largest_block", 131, 130, 1, 1, 64, 2, 1, MJ_PATCH_CHW, 0, {{3, 1, 128, 128}}, 3});
    out.push_back({"largest_block_hwc_u8", 257, 258, 1, 1, 64, 4, 1, MJ_PATCH_HWC, 0, {{1, 2, 256, 256}}, 0});
    return out;
}

int main() {
    int bad = 0, runs = 0;
    const int dtypes[4] = {MJ_DTYPE_U8, MJ_DTYPE_F16, MJ_DTYPE_BF16, MJ_DTYPE_F32}, esize[4] = {1, 2, 2, 4};
    for (const Case &cs : cases())
        for (int layout = 0; layout < 4; ++layout)
            for (int d = 0; d < 4; ++d) {
                if (cs.only_dtype >= 0 && d != cs.only_dtype) continue;
                const int es = esize[d], C = cs.C, P = cs.P, m = cs.m, t = cs.t;
                const size_t D = (size_t)C * t * P * P, sn = (size_t)cs.W * cs.H * C;
                const mj_patch_window *wins = cs.windows.empty() ? nullptr : cs.windows.data();
                int64_t rows = -1, total = 0;
                for (int k = 0; k < cs.N; ++k) total += tokens(cs, k);
                ++runs;
                if (mj_host_patchify_count(layout, dtypes[d], C, cs.W, cs.H, cs.N, P, m, t, cs.order, cs.length, wins, &rows) != MJ_OK ||
                    rows != (cs.length ? (int64_t)cs.N * cs.length : total)) {
                    ++bad;
                    fprintf(stderr, "%s: the row count: %s\n", cs.name.c_str(), mj_last_error(nullptr));
                    continue;
                }
                // exactly sized heap buffers: one element outside either is the sanitizer's
                uint8_t *src = new uint8_t[cs.N * sn * es], *dst = new uint8_t[(size_t)rows * D * es];
                uint32_t s = 99u + (uint32_t)(d * 7 + C + layout);
                for (size_t i = 0; i < cs.N * sn * es; ++i) { s = s * 1664525u + 1013904223u; src[i] = (uint8_t)(s >> 24); }       // (arbitrary bits: NaN patterns among them)
                memset(dst, 0xEE, (size_t)rows * D * es);
                std::vector<uint8_t> want((size_t)rows * D * es, 0);
                int64_t row0 = 0;
                for (int k = 0; k < cs.N; ++k) {
                    const mj_patch_window w = wins ? wins[k] : mj_patch_window{0, 0, cs.W, cs.H};
                    const int gh = w.height / P, gw = w.width / P;
                    if (cs.length) row0 = (int64_t)k * cs.length;
                    for (int py = 0; py < gh; ++py)
                        for (int px = 0; px < gw; ++px) {
                            const int64_t row = row0 + ((int64_t)(py / m) * (gw / m) + px / m) * m * m + (py % m) * m + px % m;
                            for (int c = 0; c < C; ++c)
                                for (int j = 0; j < P; ++j)
                                    for (int i = 0; i < P; ++i) {
                                        const uint8_t *from = src + (k * sn + at(layout, cs.W, cs.H, C, c, w.y + py * P + j, w.x + px * P + i)) * es;
                                        if (cs.order == MJ_PATCH_HWC) memcpy(&want[((size_t)row * D + ((size_t)j * P + i) * C + c) * es], from, es);
                                        else
                                            for (int r = 0; r < t; ++r) memcpy(&want[((size_t)row * D + (((size_t)c * t + r) * P + j) * P + i) * es], from, es);
                                    }
                        }
                    if (!cs.length) row0 += (int64_t)gh * gw;
                }
                ++runs;
                const int rc = mj_host_patchify(src, dst, layout, dtypes[d], C, cs.W, cs.H, cs.N, P, m, t, cs.order, cs.length, wins);
                if (rc != MJ_OK) { ++bad; fprintf(stderr, "refused: %s\n", mj_last_error(nullptr)); }
                else if (memcmp(dst, want.data(), want.size())) {
                    ++bad;
                    fprintf(stderr, "%s: layout %d dtype %d: differs from the rule\n", cs.name.c_str(), layout, dtypes[d]);
                }
                delete[] src;
                delete[] dst;
            }
    // refusals, which write nothing
    {
        std::vector<uint8_t> a(2 * 8 * 6 * 3, 9), b(2 * 12 * 12, 4);
        mj_patch_window w[2] = {{0, 0, 8, 6}, {2, 0, 8, 6}};
        ++runs;
        if (mj_host_patchify(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 8, 6, 2, 2, 1, 1, MJ_PATCH_CHW, 0, w) != MJ_ERR_INVALID) ++bad;
        w[1] = mj_patch_window{0, 0, 6, 6};
        if (mj_host_patchify(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 8, 6, 2, 2, 2, 1, MJ_PATCH_CHW, 0, w) != MJ_ERR_INVALID) ++bad;
        if (mj_host_patchify(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 8, 6, 2, 4, 1, 1, MJ_PATCH_CHW, 0, nullptr) != MJ_ERR_INVALID) ++bad;
        if (mj_host_patchify(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 8, 6, 2, 2, 1, 2, MJ_PATCH_HWC, 0, nullptr) != MJ_ERR_INVALID) ++bad;
        if (mj_host_patchify(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 8, 6, 2, 2, 1, 1, MJ_PATCH_CHW, 11, nullptr) != MJ_ERR_INVALID) ++bad;
        if (mj_host_patchify(a.data(), a.data() + 8, MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 8, 6, 1, 2, 1, 1, MJ_PATCH_CHW, 0, nullptr) != MJ_ERR_INVALID) ++bad;
        for (uint8_t v : b) if (v != 4) { ++bad; break; }
        if (mj_host_patchify(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 8, 6, 2, 2, 1, 1, MJ_PATCH_CHW, 0, nullptr) != MJ_OK) ++bad;
        for (uint8_t v : b) if (v != 9) { ++bad; break; }
    }
    printf("patch_host_check: %d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
