// Stand-alone check of the erase launch's host twin (mj_host_erase) for a sanitizer build of the library's host code: no GPU, no
// Python.  The address arithmetic is the kernel's (csrc/erase_addr.h: erase_run, one function for both), so what AddressSanitizer
// sees here — every element a box addresses, in every layout, element size and component count, on EXACTLY sized heap buffers, the
// blocks of values exactly sized too — is what every lane of k_erase addresses.  The box list is that of tests/test_erase_host.py:
// 1 x 1, 1 x h, w x 1, the whole canvas, each corner, an odd x with an odd width, two disjoint boxes, two overlapping ones in both
// orders — in the first and in the last slot.  Every result is held to a plain restatement of the rule on (C, H, W) coordinates.
//
//   make -C pyjpegdecoder_amd/csrc XFLAGS="-Xarch_host -fsanitize=address,undefined" OUT=$PWD/build_san/libmijpeg_san.so OBJDIR=$PWD/build_san/obj
//   hipcc -std=c++17 -fsanitize=address,undefined -Iinclude tools/erase_host_check.cpp -Lbuild_san -lmijpeg_san -Wl,-rpath,$PWD/build_san -o build_san/erase_host_check
//   UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 build_san/erase_host_check
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

int main() {
    int bad = 0, runs = 0;
    const int sizes[2][2] = {{23, 17}, {40, 28}};
    const int dtypes[4] = {MJ_DTYPE_U8, MJ_DTYPE_F16, MJ_DTYPE_BF16, MJ_DTYPE_F32}, esize[4] = {1, 2, 2, 4};
    for (const auto &sz : sizes) {
        const int W = sz[0], H = sz[1];
        const std::vector<std::vector<Box>> cases = {
            {{4, 3, 1, 1}}, {{3, 2, 1, H - 4}}, {{2, 3, W - 4, 1}}, {{0, 0, W, H}}, {{0, 0, 3, 2}}, {{W - 3, 0, 3, 2}}, {{0, H - 2, 3, 2}},
            {{W - 3, H - 2, 3, 2}}, {{5, 4, 7, 5}}, {{1, 1, 4, 3}, {10, 8, 5, 4}}, {{2, 2, 8, 6}, {6, 5, 9, 7}}, {{6, 5, 9, 7}, {2, 2, 8, 6}}};
        for (int layout = 0; layout < 4; ++layout)
            for (int d = 0; d < 4; ++d)
                for (int C : {1, 3})
                    for (const auto &boxes : cases)
                        for (int slot : {0, 2}) {
                            const int es = esize[d], n_slots = 3;
                            const size_t n = (size_t)W * H * C;
                            // the array and the model, byte for byte: every element's bytes are its index's low bytes
                            std::vector<uint8_t> arr(n_slots * n * es), want;
                            for (size_t i = 0; i < arr.size(); ++i) arr[i] = (uint8_t)(i * 7 + 1);
                            want = arr;
                            std::vector<mj_erase_rect> rects;
                            std::vector<uint8_t> values;
                            for (size_t j = 0; j < boxes.size(); ++j) {
                                const Box &b = boxes[j];
                                mj_erase_rect r{};
                                r.output = slot; r.x = b.x; r.y = b.y; r.width = b.w; r.height = b.h;
                                if ((j + layout + d) & 1) {            // values: a (C, h, w) block, its bytes a pattern of its own
                                    r.kind = MJ_ERASE_VALUES;
                                    r.offset = (int64_t)(values.size() / es);
                                    const size_t m = (size_t)C * b.w * b.h * es;
                                    for (size_t i = 0; i < m; ++i) values.push_back((uint8_t)(200 - i * 3 - j));
                                    for (int c = 0; c < C; ++c)
                                        for (int y = 0; y < b.h; ++y)
                                            for (int x = 0; x < b.w; ++x)
                                                memcpy(&want[(slot * n + at(layout, W, H, C, c, b.y + y, b.x + x)) * es],
                                                       &values[((size_t)r.offset + ((size_t)c * b.h + y) * b.w + x) * es], es);
                                } else {                                // a constant: small integers, exact in every type
                                    r.kind = MJ_ERASE_CONST;
                                    for (int c = 0; c < C; ++c) r.value[c] = (float)(2 + c + 4 * j);
                                    for (int c = 0; c < C; ++c) {
                                        const float f = r.value[c];
                                        uint32_t bits;
                                        memcpy(&bits, &f, 4);
                                        uint8_t e[4] = {0, 0, 0, 0};
                                        if (dtypes[d] == MJ_DTYPE_U8) e[0] = (uint8_t)f;
                                        else if (dtypes[d] == MJ_DTYPE_F32) memcpy(e, &bits, 4);
                                        else if (dtypes[d] == MJ_DTYPE_BF16) { const uint16_t h = (uint16_t)(bits >> 16); memcpy(e, &h, 2); }
                                        else {                          // float16 of a small integer: exponent rebias, mantissa cut (exact)
                                            const uint16_t h = (uint16_t)((((bits >> 23) - 112) << 10) | ((bits >> 13) & 0x3FF));
                                            memcpy(e, &h, 2);
                                        }
                                        for (int y = 0; y < b.h; ++y)
                                            for (int x = 0; x < b.w; ++x)
                                                memcpy(&want[(slot * n + at(layout, W, H, C, c, b.y + y, b.x + x)) * es], e, es);
                                    }
                                }
                                rects.push_back(r);
                            }
                            ++runs;
                            // exactly sized heap copies: one element outside the array or the values is the sanitizer's
                            uint8_t *heap = new uint8_t[arr.size()];
                            memcpy(heap, arr.data(), arr.size());
                            uint8_t *vheap = values.empty() ? nullptr : new uint8_t[values.size()];
                            if (vheap) memcpy(vheap, values.data(), values.size());
                            const int rc = mj_host_erase(heap, layout, dtypes[d], C, W, H, n_slots, (int32_t)rects.size(), rects.data(), vheap);
                            if (rc != MJ_OK) { ++bad; fprintf(stderr, "refused: %s\n", mj_last_error(nullptr)); }
                            else if (memcmp(heap, want.data(), want.size())) {
                                ++bad;
                                fprintf(stderr, "layout %d dtype %d C %d %dx%d slot %d: differs from the rule\n", layout, dtypes[d], C, W, H, slot);
                            }
                            delete[] heap;
                            delete[] vheap;
                        }
    }
    // refusals leave the array alone
    {
        std::vector<uint8_t> a(6 * 5 * 3, 9);
        mj_erase_rect r{};
        r.width = 7; r.height = 1;
        if (mj_host_erase(a.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 6, 5, 1, 1, &r, nullptr) != MJ_ERR_INVALID) ++bad;
        r.width = 1; r.output = 1;
        if (mj_host_erase(a.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 6, 5, 1, 1, &r, nullptr) != MJ_ERR_INVALID) ++bad;
        r.output = 0; r.kind = MJ_ERASE_VALUES;
        if (mj_host_erase(a.data(), MJ_LAYOUT_ROWMAJOR, MJ_DTYPE_U8, 3, 6, 5, 1, 1, &r, nullptr) != MJ_ERR_INVALID) ++bad;
        for (uint8_t v : a) if (v != 9) { ++bad; break; }
    }
    printf("erase_host_check: %d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
