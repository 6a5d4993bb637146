// Stand-alone check of the compose launch's host twin (mj_host_compose) for a sanitizer build of the library's host code: no GPU, no
// Python.  The resolve and the job list are the launch's own (csrc/compose_addr.h, one set of functions for both), so what
// AddressSanitizer and the undefined-behaviour sanitizer see here — every element read and written, in every layout, element size and
// component count, on EXACTLY sized heap buffers — is what the lanes of k_compose address.  The tile lists are those of
// tests/compose_cases.py: a tile whole, one-pixel windows at the corners, an odd window, tiles clipped at every side and at corners,
// tiles wholly outside, an empty entry, an exact cover, chains of three in both orders, a source twice, the 8 x 8 grid of 64 tiles
// with gutters, three different fills.  Every result is held to a plain restatement of the rule — paste in order — on (c, y, x)
// coordinates, and mj_host_compose_resolve's rectangles are counted over the canvas: every pixel once.
//
//   make -C pyjpegdecoder_amd/csrc XFLAGS="-Xarch_host -fsanitize=address,undefined" OUT=$PWD/build_san/libmijpeg_san.so OBJDIR=$PWD/build_san/obj
//   hipcc -std=c++17 -fsanitize=address,undefined -Iinclude tools/compose_host_check.cpp -Lbuild_san -lmijpeg_san -Wl,-rpath,$PWD/build_san -o build_san/compose_host_check
//   UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 build_san/compose_host_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mijpeg.h"

typedef std::vector<mj_compose_tile> Tiles;

// element offset of (c, y, x) inside one W x H slot
static size_t at(int layout, int W, int H, int C, int c, int y, int x) {
    switch (layout) {
        case MJ_LAYOUT_XMAJOR: return ((size_t)x * H + y) * C + c;
        case MJ_LAYOUT_ROWMAJOR: return ((size_t)y * W + x) * C + c;
        case MJ_LAYOUT_PLANAR_XMAJOR: return ((size_t)c * W + x) * H + y;
        default: return ((size_t)c * H + y) * W + x;
    }
}

static mj_compose_tile tile(int output, int source, int dx, int dy, int sx, int sy, int w, int h) { return mj_compose_tile{output, source, sx, sy, w, h, dx, dy}; }

struct Case {
    const char *name;
    int sw, sh, dw, dh, n_outputs;
    Tiles tiles;
};

static std::vector<Case> cases() {
    std::vector<Case> out;
    const int geo[2][4] = {{13, 9, 21, 14}, {24, 16, 37, 23}};
    for (const auto &g : geo) {
        const int SW = g[0], SH = g[1], W = g[2], H = g[3];
        auto whole = [&](int m, int s, int dx, int dy) { return tile(m, s, dx, dy, 0, 0, SW, SH); };
        out.push_back({"whole", SW, SH, W, H, 1, {whole(0, 0, 3, 2)}});
        out.push_back({"corner_pixels", SW, SH, W, H, 1, {tile(0, 0, 0, 0, 0, 0, 1, 1), tile(0, 1, W - 1, 0, SW - 1, 0, 1, 1), tile(0, 2, 0, H - 1, 0, SH - 1, 1, 1),
                                                         tile(0, 3, W - 1, H - 1, SW - 1, SH - 1, 1, 1)}});
        out.push_back({"odd_window", SW, SH, W, H, 1, {tile(0, 1, 5, 3, 3, 1, 7, 5)}});
        out.push_back({"clipped", SW, SH, W, H, 6, {whole(0, 0, -4, 2), whole(1, 1, W - 5, 2), whole(2, 2, 3, -3), whole(3, 3, 3, H - 4), whole(4, 0, -6, -5), whole(5, 1, W - 3, H - 2)}});
        out.push_back({"outside_and_empty", SW, SH, W, H, 5, {whole(0, 0, W, 0), whole(1, 1, -SW, 3), whole(2, 2, 3, H + 5), whole(3, 3, 3, -SH)}});
        out.push_back({"exact_cover", SW, SH, W, H, 1, {whole(0, 0, 0, 0), tile(0, 1, SW, 0, 0, 0, W - SW, SH), tile(0, 2, 0, SH, 0, 0, SW, H - SH), tile(0, 3, SW, SH, 2, 1, W - SW, H - SH)}});
        out.push_back({"chain", SW, SH, W, H, 1, {tile(0, 0, 1, 1, 0, 0, 9, 6), tile(0, 1, 5, 4, 2, 1, 9, 6), tile(0, 2, 9, 7, 4, 3, 9, 6)}});
        out.push_back({"chain_reversed", SW, SH, W, H, 1, {tile(0, 2, 9, 7, 4, 3, 9, 6), tile(0, 1, 5, 4, 2, 1, 9, 6), tile(0, 0, 1, 1, 0, 0, 9, 6)}});
        out.push_back({"twice_in_one", SW, SH, W, H, 1, {tile(0, 0, 0, 0, 0, 0, 6, 5), tile(0, 0, 8, 6, 3, 2, 7, 6)}});
        // (the tiles of two outputs interleaved: they need not be grouped)
        out.push_back({"twice_in_two", SW, SH, W, H, 2, {tile(1, 1, 4, 1, 1, 1, 5, 5), whole(0, 1, 2, 2)}});
        out.push_back({"three_fills", SW, SH, W, H, 2, {tile(0, 2, 6, 4, 1, 2, 5, 3)}});
    }
    Tiles grid;
    for (int k = 0; k < 64; ++k) grid.push_back(tile(0, k % 4, 1 + 5 * (k % 8), 1 + 4 * (k / 8), k % 10, k % 7, 4, 3));
    out.push_back({"grid64", 13, 9, 41, 33, 1, grid});
    return out;
}

int main() {
    int bad = 0, runs = 0;
    const int dtypes[4] = {MJ_DTYPE_U8, MJ_DTYPE_F16, MJ_DTYPE_BF16, MJ_DTYPE_F32}, esize[4] = {1, 2, 2, 4};
    const uint32_t fills[3][3] = {{0xA5, 0x3C, 0x7F}, {0x7E01, 0x3C00, 0xFBFF}, {0x7FC00001u, 0x3F800000u, 0xFF7FFFFFu}};
    const int N = 5;        // sources; the last is never named
    for (const Case &cs : cases())
        for (int layout = 0; layout < 4; ++layout) {
            // the rectangles: inside the canvas, and every pixel of every output in exactly one
            {
                int32_t cap = 0, n = 0;
                ++runs;
                if (mj_host_compose_resolve(layout, 3, cs.sw, cs.sh, N, cs.dw, cs.dh, cs.n_outputs, (int32_t)cs.tiles.size(), cs.tiles.data(), nullptr, 0, &cap) != MJ_OK) { ++bad; continue; }
                mj_compose_rect *rects = new mj_compose_rect[cap];          // (exactly the capacity reported)
                if (mj_host_compose_resolve(layout, 3, cs.sw, cs.sh, N, cs.dw, cs.dh, cs.n_outputs, (int32_t)cs.tiles.size(), cs.tiles.data(), rects, cap, &n) != MJ_OK || n >= cap) ++bad;
                else {
                    std::vector<int> seen((size_t)cs.n_outputs * cs.dw * cs.dh, 0);
                    for (int i = 0; i < n; ++i) {
                        const mj_compose_rect &r = rects[i];
                        if (r.output < 0 || r.output >= cs.n_outputs || r.x < 0 || r.y < 0 || r.width < 1 || r.height < 1 || r.x + r.width > cs.dw || r.y + r.height > cs.dh) { ++bad; break; }
                        for (int y = r.y; y < r.y + r.height; ++y)
                            for (int x = r.x; x < r.x + r.width; ++x) ++seen[((size_t)r.output * cs.dh + y) * cs.dw + x];
                    }
                    for (int v : seen) if (v != 1) { ++bad; fprintf(stderr, "%s layout %d: the rectangles are no partition\n", cs.name, layout); break; }
                }
                delete[] rects;
            }
            for (int d = 0; d < 4; ++d)
                for (int C : {1, 3}) {
                    const int es = esize[d];
                    const size_t sn = (size_t)cs.sw * cs.sh * C, dn = (size_t)cs.dw * cs.dh * C;
                    // exactly sized heap buffers: one element outside either is the sanitizer's
                    uint8_t *src = new uint8_t[N * sn * es], *dst = new uint8_t[cs.n_outputs * dn * es];
                    uint32_t s = 99u + (uint32_t)(d * 7 + C + layout);
                    for (size_t i = 0; i < N * sn * es; ++i) { s = s * 1664525u + 1013904223u; src[i] = (uint8_t)(s >> 24); }       // (arbitrary bits: NaN patterns among them)
                    memset(dst, 0xEE, cs.n_outputs * dn * es);
                    const uint32_t *fill = fills[es == 1 ? 0 : es == 2 ? 1 : 2];
                    std::vector<uint8_t> want(cs.n_outputs * dn * es);
                    for (int m = 0; m < cs.n_outputs; ++m)
                        for (int c = 0; c < C; ++c)
                            for (int y = 0; y < cs.dh; ++y)
                                for (int x = 0; x < cs.dw; ++x) memcpy(&want[(m * dn + at(layout, cs.dw, cs.dh, C, c, y, x)) * es], &fill[c], es);       // (little-endian: the low bytes)
                    for (const mj_compose_tile &t : cs.tiles)
                        for (int c = 0; c < C; ++c)
                            for (int y = 0; y < t.height; ++y)
                                for (int x = 0; x < t.width; ++x) {
                                    const int X = t.dx + x, Y = t.dy + y;
                                    if (X < 0 || Y < 0 || X >= cs.dw || Y >= cs.dh) continue;
                                    memcpy(&want[(t.output * dn + at(layout, cs.dw, cs.dh, C, c, Y, X)) * es],
                                           src + (t.source * sn + at(layout, cs.sw, cs.sh, C, c, t.sy + y, t.sx + x)) * es, es);
                                }
                    ++runs;
                    const int rc = mj_host_compose(src, dst, layout, dtypes[d], C, cs.sw, cs.sh, N, cs.dw, cs.dh, cs.n_outputs, fill, (int32_t)cs.tiles.size(),
                                                   cs.tiles.empty() ? nullptr : cs.tiles.data());
                    if (rc != MJ_OK) { ++bad; fprintf(stderr, "refused: %s\n", mj_last_error(nullptr)); }
                    else if (memcmp(dst, want.data(), want.size())) {
                        ++bad;
                        fprintf(stderr, "%s: layout %d dtype %d C %d: differs from the rule\n", cs.name, layout, dtypes[d], C);
                    }
                    delete[] src;
                    delete[] dst;
                }
        }
    // no tiles at all, and refusals, which write nothing
    {
        std::vector<uint8_t> a(2 * 6 * 5 * 3, 9), b(1 * 8 * 7 * 3, 4);
        const uint32_t fill[3] = {1, 2, 3};
        ++runs;
        if (mj_host_compose(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 6, 5, 2, 8, 7, 1, fill, 0, nullptr) != MJ_OK) ++bad;
        for (size_t i = 0; i < b.size(); ++i) if (b[i] != 1 + i % 3) { ++bad; break; }
        std::fill(b.begin(), b.end(), 4);
        mj_compose_tile t = tile(0, 0, 0, 0, 0, 0, 7, 1);
        if (mj_host_compose(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 6, 5, 2, 8, 7, 1, fill, 1, &t) != MJ_ERR_INVALID) ++bad;
        t = tile(0, 2, 0, 0, 0, 0, 1, 1);
        if (mj_host_compose(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 6, 5, 2, 8, 7, 1, fill, 1, &t) != MJ_ERR_INVALID) ++bad;
        t = tile(1, 0, 0, 0, 0, 0, 1, 1);
        if (mj_host_compose(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 6, 5, 2, 8, 7, 1, fill, 1, &t) != MJ_ERR_INVALID) ++bad;
        t = tile(0, 0, 1 << 20, 0, 0, 0, 1, 1);
        if (mj_host_compose(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 6, 5, 2, 8, 7, 1, fill, 1, &t) != MJ_ERR_INVALID) ++bad;
        t = tile(0, 0, 0, 0, 0, 0, 1, 1);
        if (mj_host_compose(a.data(), a.data() + 8, MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 6, 5, 1, 4, 4, 1, fill, 1, &t) != MJ_ERR_INVALID) ++bad;
        for (uint8_t v : b) if (v != 4) { ++bad; break; }
    }
    printf("compose_host_check: %d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
