// Stand-alone check of the mix launch's host twin (mj_host_mix) for a sanitizer build of the library's host code: no GPU, no Python.
// The rule and the box test are the kernel's (csrc/mix_rule.h, one set of functions for both), so what AddressSanitizer and the
// undefined-behaviour sanitizer see here — every element read and written, in every layout, element size and component count, on
// EXACTLY sized heap buffers — is what the lanes of k_mix compute and address.  The case list is that of tests/mix_cases.py: the roll,
// flip, self and 3-cycle pairings, the lam values 0, 1, 0.3, 0.5, a Beta draw and 1e-5, and the single boxes — 1 x 1, 1 x h, w x 1,
// the whole canvas, each corner, an odd x with an odd width.  CutMix and copied outputs are held to a plain restatement of the rule
// on (C, H, W) coordinates; MixUp to float arithmetic on values every type holds exactly (small integers, lam 0.5 and 0.25).
//
//   make -C pyjpegdecoder_amd/csrc XFLAGS="-Xarch_host -fsanitize=address,undefined" OUT=$PWD/build_san/libmijpeg_san.so OBJDIR=$PWD/build_san/obj
//   hipcc -std=c++17 -fsanitize=address,undefined -Iinclude tools/mix_host_check.cpp -Lbuild_san -lmijpeg_san -Wl,-rpath,$PWD/build_san -o build_san/mix_host_check
//   UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 build_san/mix_host_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mijpeg.h"

struct Box { int x, y, w, h; };

// element offset of (c, y, x) inside one slot
static size_t at(int layout, int W, int H, int C, int c, int y, int x) {
    switch (layout) {
        case MJ_LAYOUT_XMAJOR: return ((size_t)x * H + y) * C + c;
        case MJ_LAYOUT_ROWMAJOR: return ((size_t)y * W + x) * C + c;
        case MJ_LAYOUT_PLANAR_XMAJOR: return ((size_t)c * W + x) * H + y;
        default: return ((size_t)c * H + y) * W + x;
    }
}

// a small integer 0..63 as an element of the dtype (exact in all of them)
static void put(uint8_t *e, int dtype, int v) {
    const float f = (float)v;
    uint32_t bits;
    memcpy(&bits, &f, 4);
    if (dtype == MJ_DTYPE_U8) e[0] = (uint8_t)v;
    else if (dtype == MJ_DTYPE_F32) memcpy(e, &bits, 4);
    else if (dtype == MJ_DTYPE_BF16) { const uint16_t h = (uint16_t)(bits >> 16); memcpy(e, &h, 2); }
    else { const uint16_t h = v ? (uint16_t)((((bits >> 23) - 112) << 10) | ((bits >> 13) & 0x3FF)) : 0; memcpy(e, &h, 2); }
}

int main() {
    int bad = 0, runs = 0;
    const int sizes[2][2] = {{23, 17}, {24, 16}};
    const int dtypes[4] = {MJ_DTYPE_U8, MJ_DTYPE_F16, MJ_DTYPE_BF16, MJ_DTYPE_F32}, esize[4] = {1, 2, 2, 4};
    const double lams[6] = {0.0, 1.0, 0.3, 0.5, 0.24372071077733867, 1e-5};     // (mix_cases.beta_draw()'s value)
    const int N = 5;
    const int pairings[4][5] = {{4, 0, 1, 2, 3}, {4, 3, 2, 1, 0}, {0, 1, 2, 3, 4}, {2, 0, 1, 4, 3}};
    for (const auto &sz : sizes) {
        const int W = sz[0], H = sz[1];
        const std::vector<Box> boxes = {{4, 3, 1, 1}, {3, 2, 1, H - 4}, {2, 3, W - 4, 1}, {0, 0, W, H}, {0, 0, 3, 2}, {W - 3, 0, 3, 2}, {0, H - 2, 3, 2},
                                        {W - 3, H - 2, 3, 2}, {5, 4, 7, 5}};
        for (int layout = 0; layout < 4; ++layout)
            for (int d = 0; d < 4; ++d)
                for (int C : {1, 3})
                    for (int pr = 0; pr < 4; ++pr)
                        for (size_t first = 0; first < boxes.size(); first += 3) {
                            const int es = esize[d], dtype = dtypes[d];
                            const size_t n = (size_t)W * H * C;
                            // exactly sized heap buffers: one element outside either is the sanitizer's
                            uint8_t *src = new uint8_t[N * n * es], *dst = new uint8_t[N * n * es];
                            std::vector<int> val(N * n);
                            for (size_t i = 0; i < N * n; ++i) { val[i] = (int)((i * 7 + i / n) % 61); put(src + i * es, dtype, val[i]); }
                            memset(dst, 0xEE, N * n * es);
                            std::vector<uint8_t> want(src, src + N * n * es);
                            mj_mix_op ops[N];
                            for (int k = 0; k < N; ++k) {
                                mj_mix_op &o = ops[k];
                                o = mj_mix_op{};
                                o.partner = pairings[pr][k];
                                const int kind = (k + (int)first) % 3;     // cutmix / mixup (floats) / none in turn
                                if (kind == 2) { o.kind = MJ_MIX_NONE; o.partner = -7; continue; }      // (ignored where nothing is mixed)
                                if (kind == 1 && dtype != MJ_DTYPE_U8) {
                                    // lam 0.5 and 0.25 on small integers: products and sums exact in every float type
                                    o.kind = MJ_MIX_MIXUP;
                                    o.lam = (k & 1) ? 0.5 : 0.25;
                                    for (size_t e = 0; e < n; ++e) {
                                        const float r = (float)val[o.partner * n + e] * (float)(1.0 - o.lam) + (float)val[k * n + e] * (float)o.lam;
                                        // (quarters of integers below 64: 8 significant bits at the most, bfloat16 holds them)
                                        uint32_t bits;
                                        memcpy(&bits, &r, 4);
                                        uint8_t *w = &want[(k * n + e) * es];
                                        if (dtype == MJ_DTYPE_F32) memcpy(w, &bits, 4);
                                        else if (dtype == MJ_DTYPE_BF16) { const uint16_t h = (uint16_t)(bits >> 16); memcpy(w, &h, 2); }
                                        else { const uint16_t h = r != 0.f ? (uint16_t)((((bits >> 23) - 112) << 10) | ((bits >> 13) & 0x3FF)) : 0; memcpy(w, &h, 2); }
                                    }
                                    continue;
                                }
                                const Box &b = boxes[(first + k) % boxes.size()];
                                o.kind = MJ_MIX_CUTMIX; o.x = b.x; o.y = b.y; o.width = b.w; o.height = b.h;
                                for (int c = 0; c < C; ++c)
                                    for (int y = 0; y < b.h; ++y)
                                        for (int x = 0; x < b.w; ++x) {
                                            const size_t e = at(layout, W, H, C, c, b.y + y, b.x + x);
                                            memcpy(&want[(k * n + e) * es], src + (o.partner * n + e) * es, es);
                                        }
                            }
                            ++runs;
                            const int rc = mj_host_mix(src, dst, layout, dtype, C, W, H, N, ops);
                            if (rc != MJ_OK) { ++bad; fprintf(stderr, "refused: %s\n", mj_last_error(nullptr)); }
                            else if (memcmp(dst, want.data(), want.size())) {
                                ++bad;
                                fprintf(stderr, "layout %d dtype %d C %d %dx%d pairing %d boxes from %zu: differs from the rule\n", layout, dtype, C, W, H, pr, first);
                            }
                            delete[] src;
                            delete[] dst;
                        }
        // every lam over arbitrary bit patterns (NaN, infinities and subnormals among them): the conversions' every path, results unchecked
        for (int d = 1; d < 4; ++d)
            for (double lam : lams) {
                const int es = esize[d];
                const size_t n = (size_t)W * H * 3;
                uint8_t *src = new uint8_t[2 * n * es], *dst = new uint8_t[2 * n * es];
                uint32_t s = 12345u + (uint32_t)d;
                for (size_t i = 0; i < 2 * n * es; ++i) { s = s * 1664525u + 1013904223u; src[i] = (uint8_t)(s >> 24); }
                mj_mix_op ops[2] = {};
                ops[0].kind = ops[1].kind = MJ_MIX_MIXUP;
                ops[0].partner = 1; ops[1].partner = 1;
                ops[0].lam = ops[1].lam = lam;
                ++runs;
                if (mj_host_mix(src, dst, MJ_LAYOUT_ROWMAJOR, dtypes[d], 3, W, H, 2, ops) != MJ_OK) { ++bad; fprintf(stderr, "refused: %s\n", mj_last_error(nullptr)); }
                delete[] src;
                delete[] dst;
            }
    }
    // refusals write nothing
    {
        std::vector<uint8_t> a(2 * 6 * 5 * 3, 9), b(2 * 6 * 5 * 3, 4);
        mj_mix_op ops[2] = {};
        ops[1].kind = MJ_MIX_CUTMIX; ops[1].width = 7; ops[1].height = 1;
        if (mj_host_mix(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 6, 5, 2, ops) != MJ_ERR_INVALID) ++bad;
        ops[1].width = 1; ops[1].partner = 2;
        if (mj_host_mix(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 6, 5, 2, ops) != MJ_ERR_INVALID) ++bad;
        ops[1].partner = 0; ops[1].kind = MJ_MIX_MIXUP; ops[1].lam = 0.5;
        if (mj_host_mix(a.data(), b.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 6, 5, 2, ops) != MJ_ERR_INVALID) ++bad;
        if (mj_host_mix(a.data(), a.data() + 8, MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 6, 5, 1, ops) != MJ_ERR_INVALID) ++bad;
        for (uint8_t v : b) if (v != 4) { ++bad; break; }
    }
    printf("mix_host_check: %d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
