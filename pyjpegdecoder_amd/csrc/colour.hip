// Colour operations (mj_plan_request.colour): what one call of Pillow's ImageEnhance.* / ImageOps.* does to
// the bytes of the finished canvas, between the resize launch and the mirror and element type of the output.  The resize launch
// of such a plan writes uint8 canvases, unmirrored, output after output, into a plan-owned buffer; the launches here take every
// output through its chain, step by step, and store the last step into the caller's array (resize_plan.hip: colour_stage).
//
// The arithmetic is Pillow's (tools/colour_model.py restates it; include/mijpeg.h has the rules), and it is written once, in
// mijpeg_internal.h, for the kernels and for the host twin (mj_host_colour_ops): colour_blend, colour_smooth,
// colour_table_entry, blur_pixel, colour_hue.  float32 and double operations round one by one (the library is compiled with -ffp-contract=off).
//
// Per step s of the plan's longest chain, up to three launches, and one more (or one per pass) where a chain blurs:
//   k_colour_hist    only where some output's op s is contrast, autocontrast or equalize, over those outputs: a workgroup counts
//                    kColourHistPixels pixels of one canvas into 4 x 256 32-bit bins in LDS (components 0..2 and L) with LDS
//                    atomics — a lane takes consecutive pixels and adds once per run of one value — and adds the bins that are
//                    not empty to the output's uint32[4][256] in global memory, which the plan zeroed on the stream just before
//   k_colour_tables  only where some output's op s is a table: one wavefront per output builds uint8[3][256]; ops with statistics
//                    scan their 256 bins in LDS, one lane per histogram (colour_scan), then every lane makes its entries
//   k_colour_apply   one thread per pixel, all its components: the output's table, color, sharpness (the 3 x 3 neighbourhood of
//                    the source canvas, edges copied), or a copy where the chain has ended.  Steps go from one canvas to the
//                    other (sharpness cannot run in place); the last step stores at the output's slot, column ow - 1 - x where the
//                    output is mirrored, through the output table in the plan's element type
//   k_colour_blur    only where some output's op s is gaussian_blur or box_blur, over those outputs, which k_colour_apply leaves out:
//                    a workgroup holds one component plane of one output in LDS and runs all the passes there; on plans whose canvas
//                    LDS does not hold, k_colour_blur_pass instead, one launch per pass through a third canvas (further down)
//   k_colour_hue     only where some output of three components has adjust_hue as its op s, over those outputs, which k_colour_apply
//                    leaves out as it does blur outputs: four neighbouring pixels per lane through colour_hue (further down)
// Everything addresses a canvas through a pixel's place p and two strides (DevColourOutput's comment), so that one kernel serves
// the four layouts.  The statistics never leave the device and nothing waits for the host.
#include <math.h>

#include "plan.h"

namespace mj {

namespace {

// one histogram, scanned: prefix[i] = the sum of h below i; the first and last non-empty bins, how many there are, the last
// one's count, the sum of all, and the weighted sum (contrast's mean is wsum / total)
__host__ __device__ inline void colour_scan(const uint32_t *h, unsigned long long *prefix, ColourStats &st, unsigned long long &wsum) {
    st.lo = 256; st.hi = -1; st.nz = 0; st.last = 0; st.total = 0; st.mean = 0;
    wsum = 0;
    for (int i = 0; i < 256; ++i) {
        const unsigned long long v = h[i];
        prefix[i] = st.total;
        if (v) {
            if (st.lo == 256) st.lo = i;
            st.hi = i; st.last = v; ++st.nz;
        }
        st.total += v;
        wsum += v * (unsigned long long)i;
    }
}
__host__ __device__ inline int colour_mean(unsigned long long wsum, unsigned long long total) {
    return total ? (int)((double)wsum / (double)total + 0.5) : 0;
}

// workgroup `wg` of a launch whose grid is (x, y): launches number their workgroups as launch_resize does
__device__ inline int64_t workgroup_index() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }

template <int C>
__global__ __launch_bounds__(256) void k_colour_hist(const ColourArgs a, const int step) {
    __shared__ uint32_t bins[4 * 256];
    const int64_t npix = (int64_t)a.ow * a.oh, chunks = (npix + kColourHistPixels - 1) / kColourHistPixels;
    const int64_t wg = workgroup_index();
    const int first = a.hist_first[step], n_list = a.hist_first[step + 1] - first;
    if (wg >= n_list * chunks) return;
    const int k = a.hist_list[first + (int)(wg / chunks)];
    const int64_t p0 = (wg % chunks) * kColourHistPixels;
    const int t = threadIdx.x;
    for (int b = 0; b < 4; ++b) bins[b * 256 + t] = 0;
    __syncthreads();
    const unsigned char *src = a.canvas[step & 1] + (int64_t)k * npix * C;
    const int64_t ps = a.layout >= 2 ? 1 : C, cs = a.layout >= 2 ? npix : 1;
    // A lane counts kColourHistPixels / 256 CONSECUTIVE pixels and merges runs of one value before it touches LDS: on a flat or
    // padded canvas every lane of the workgroup adds to the same bin, and the adds to one address serialise — one add per run
    // instead of one per pixel (1024 letterboxed 224 x 224 canvases: 0.4 ms per launch without the merge)
    constexpr int kPerLane = kColourHistPixels / 256, kBands = C == 3 ? 4 : 1;
    unsigned last[kBands], run[kBands];
    for (int b = 0; b < kBands; ++b) { last[b] = 0; run[b] = 0; }
    for (int i = 0; i < kPerLane; ++i) {
        const int64_t p = p0 + (int64_t)t * kPerLane + i;
        if (p >= npix) break;
        unsigned v[kBands];
        for (int c = 0; c < C; ++c) v[c] = src[p * ps + c * cs];
        if constexpr (C == 3) v[3] = mode_luma(v[0], v[1], v[2]);
        for (int b = 0; b < kBands; ++b) {
            if (run[b] && v[b] != last[b]) { atomicAdd(&bins[b * 256 + last[b]], run[b]); run[b] = 0; }
            last[b] = v[b]; ++run[b];
        }
    }
    for (int b = 0; b < kBands; ++b)
        if (run[b]) atomicAdd(&bins[b * 256 + last[b]], run[b]);
    __syncthreads();
    uint32_t *out = a.hist + (int64_t)k * 1024;
    for (int b = 0; b < 4; ++b) {
        const uint32_t n = bins[b * 256 + t];
        if (n) atomicAdd(&out[b * 256 + t], n);
    }
}

template <int C>
__global__ __launch_bounds__(64) void k_colour_tables(const ColourArgs a, const int step) {
    __shared__ uint32_t h[4 * 256];
    __shared__ unsigned long long prefix[4 * 256];
    __shared__ ColourStats stats[4];
    __shared__ unsigned long long wsums[4];
    const int64_t k = workgroup_index();
    if (k >= a.n_outputs) return;
    const DevColourOutput &o = a.outputs[k];
    const int kind = step < o.n ? o.kind[step] : 0;
    if (!colour_is_table(kind)) return;
    const int lane = threadIdx.x;
    if (colour_needs_hist(kind)) {
        const uint32_t *src = a.hist + k * 1024;
        for (int i = lane; i < 1024; i += 64) h[i] = src[i];
        __syncthreads();
        // (one lane per histogram: components 0 .. C - 1, and L — which is component 0's where there is one component)
        if (lane < C || (C == 3 && lane == 3)) colour_scan(h + lane * 256, prefix + lane * 256, stats[lane], wsums[lane]);
        __syncthreads();
    }
    const int L = C == 3 ? 3 : 0;
    unsigned char *tab = a.tables + k * 768;
    for (int c = 0; c < C; ++c) {
        ColourStats st = ColourStats{};
        if (colour_needs_hist(kind)) {
            st = stats[c];
            st.mean = colour_mean(wsums[L], stats[L].total);
        }
        for (int i = lane; i < 256; i += 64)
            tab[c * 256 + i] = (unsigned char)colour_table_entry(kind, o.value[step], o.ivalue[step], i, st, colour_needs_hist(kind) ? prefix[c * 256 + i] : 0);
    }
}

// Components c0 .. c0 + N - 1 of the pixel at place p = (x, y) of output k after step `step`, values r[0 .. N - 1]: into the other
// canvas, or — the chain's last step — to the output's slot, mirrored where flagged, through the output table.  Every launch that
// ends a step stores here.
template <int C, int N>
__device__ inline void colour_store(const ColourArgs &a, const DevColourOutput &o, int step, int64_t k, int64_t p, int x, int y, int c0, const unsigned *r) {
    const int64_t npix = (int64_t)a.ow * a.oh;
    const int64_t ps = a.layout >= 2 ? 1 : C, cs = a.layout >= 2 ? npix : 1;
    if (step + 1 < a.steps) {
        unsigned char *dst = a.canvas[(step + 1) & 1] + k * npix * C;
        for (int c = 0; c < N; ++c) dst[p * ps + (c0 + c) * cs] = (unsigned char)r[c];
        return;
    }
    // the last step: to the output's slot, mirrored where flagged, through the output table
    const bool rowmajor = (a.layout & 1) != 0;
    const int xm = o.mirror ? a.ow - 1 - x : x;
    const int64_t pm = rowmajor ? (int64_t)y * a.ow + xm : (int64_t)xm * a.oh + y;
    for (int c = 0; c < N; ++c) {
        const int64_t e = o.dst_off + pm * ps + (c0 + c) * cs;
        if (a.esize == 1) static_cast<unsigned char *>(a.dst)[e] = (unsigned char)r[c];
        else if (a.esize == 2) static_cast<uint16_t *>(a.dst)[e] = static_cast<const uint16_t *>(a.lut)[(c0 + c) * 256 + r[c]];
        else static_cast<uint32_t *>(a.dst)[e] = static_cast<const uint32_t *>(a.lut)[(c0 + c) * 256 + r[c]];
    }
}

template <int C>
__global__ __launch_bounds__(256) void k_colour_apply(const ColourArgs a, const int step) {
    const int64_t npix = (int64_t)a.ow * a.oh, per_output = (npix + 255) / 256;
    const int64_t wg = workgroup_index();
    if (wg >= a.n_outputs * per_output) return;
    const int64_t k = wg / per_output, p = (wg % per_output) * 256 + threadIdx.x;
    if (p >= npix) return;
    const DevColourOutput &o = a.outputs[k];
    const int kind = step < o.n ? o.kind[step] : 0;
    const bool rowmajor = (a.layout & 1) != 0;
    const int x = rowmajor ? (int)(p % a.ow) : (int)(p / a.oh), y = rowmajor ? (int)(p / a.ow) : (int)(p % a.oh);
    const int64_t ps = a.layout >= 2 ? 1 : C, cs = a.layout >= 2 ? npix : 1;
    const unsigned char *src = a.canvas[step & 1] + k * npix * C;
    unsigned v[C], r[C];
    for (int c = 0; c < C; ++c) r[c] = v[c] = src[p * ps + c * cs];
    if (colour_is_table(kind)) {
        const unsigned char *tab = a.tables + k * 768;
        for (int c = 0; c < C; ++c) r[c] = tab[c * 256 + v[c]];
    } else if (kind == MJ_COLOUR_COLOR && C == 3) {
        const int l = (int)mode_luma(v[0], v[1], v[2]);
        for (int c = 0; c < C; ++c) r[c] = colour_blend(l, (int)v[c], o.value[step]);
    } else if (kind == MJ_COLOUR_SHARPNESS && x > 0 && y > 0 && x < a.ow - 1 && y < a.oh - 1) {
        const int64_t sx = rowmajor ? 1 : a.oh, sy = rowmajor ? a.ow : 1;
        for (int c = 0; c < C; ++c) {
            float nb[3][3];
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) nb[dy + 1][dx + 1] = (float)src[(p + dx * sx + dy * sy) * ps + c * cs];
            r[c] = colour_blend((int)colour_smooth(nb), (int)v[c], o.value[step]);
        }
    }
    // (an output whose op is a blur is the blur launch's, one of three components whose op is adjust_hue the hue launch's.  Asked
    // here, behind the loads and the op, and not on top: the code of every other output stays close to what it was; the price is
    // that such an output's pixel is read for nothing — launch_colour_t does not launch this kernel for a step whose outputs are
    // all another launch's)
    if (colour_is_elsewhere(kind, C)) return;
    colour_store<C, C>(a, o, step, k, p, x, y, 0, r);
}

// ---- adjust_hue (MJ_COLOUR_ADJUST_HUE) on three components: colour_hue of every pixel of the step's hue outputs ----------------------
// Not a branch of k_colour_apply: the op carries fp64 and three float divisions, and its registers would be charged to every output
// of every chain.  A lane takes four neighbouring pixels, places p0 .. p0 + 3 — twelve consecutive bytes of an interleaved canvas,
// four of each plane of a planar one: three dwords either way, loaded as such (an image starts at a byte offset of k * npix * 3,
// so the dwords are not aligned in general; global loads need not be) —, and stores pixel by pixel through colour_store.  The last
// lane of a canvas whose pixels are no multiple of four loads its one to three pixels byte by byte: nothing is read beyond the
// canvas.  The tables come from the plan's copy into LDS once per workgroup.
__global__ __launch_bounds__(256) void k_colour_hue(const ColourArgs a, const ColourHueArgs h, const int step) {
    __shared__ float tf[256], tfs[256];
    __shared__ uint8_t tsext[256];
    const int64_t npix = (int64_t)a.ow * a.oh, quads = (npix + 3) >> 2, per_output = (quads + 255) / 256;
    const int64_t wg = workgroup_index();
    const int first = h.first[step], n_list = h.first[step + 1] - first;
    if (wg >= n_list * per_output) return;
    const int t = threadIdx.x;
    tf[t] = h.tables->f[t]; tfs[t] = h.tables->fs[t]; tsext[t] = h.tables->sextant[t];
    __syncthreads();
    const int64_t k = h.list[first + (int)(wg / per_output)], p0 = ((wg % per_output) * 256 + t) * 4;
    if (p0 >= npix) return;
    const DevColourOutput &o = a.outputs[k];
    const int shift = o.ivalue[step];
    const bool rowmajor = (a.layout & 1) != 0, planar = a.layout >= 2;
    const unsigned char *src = a.canvas[step & 1] + k * npix * 3;
    const int n = npix - p0 < 4 ? (int)(npix - p0) : 4;
    unsigned v[4][3];
    if (n == 4) {
        uint32_t d[3];
        if (planar) for (int c = 0; c < 3; ++c) __builtin_memcpy(&d[c], src + c * npix + p0, 4);
        else __builtin_memcpy(d, src + p0 * 3, 12);
        for (int j = 0; j < 4; ++j)
            for (int c = 0; c < 3; ++c) {         // (byte j of dword c, or byte 3 j + c of the twelve: both with constant indices)
                const int byte = j * 3 + c;
                v[j][c] = (planar ? d[c] >> (8 * j) : d[byte >> 2] >> (8 * (byte & 3))) & 0xFFu;
            }
    } else {
        for (int j = 0; j < 3; ++j)
            for (int c = 0; c < 3; ++c) v[j][c] = j < n ? src[planar ? c * npix + p0 + j : (p0 + j) * 3 + c] : 0u;
        v[3][0] = v[3][1] = v[3][2] = 0;
    }
    // (x, y) of the first pixel by division, of the next ones by stepping along the stored axis
    const int len = rowmajor ? a.ow : a.oh;
    int major = (int)(p0 / len), minor = (int)(p0 % len);
    // (unrolled: the four pixels stay in registers — a rolled loop indexes v[] by a variable, which puts the array into LDS)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= n) break;
        unsigned r[3];
        colour_hue(v[j][0], v[j][1], v[j][2], shift, tf, tfs, tsext, r);
        colour_store<3, 3>(a, o, step, k, p0 + j, rowmajor ? minor : major, rowmajor ? major : minor, 0, r);
        if (++minor == len) { minor = 0; ++major; }
    }
}

// ---- the blurs (MJ_COLOUR_GAUSSIAN_BLUR, MJ_COLOUR_BOX_BLUR): passes of blur_pixel along the width, then along the height ----------
// The plane-resident launch: workgroup wg takes component wg % C of the wg / C-th output of the step's blur list.  It loads the
// plane into LDS as oh rows of `pitch` dwords (ow bytes rounded up), runs every pass from one LDS plane to the other — a lane takes
// one dword, four neighbouring pixels of a row, in both directions: along the width it slides the window over its four pixels, along
// the height it sums the same dword of the rows y - r .. y + r, byte by byte —, and stores the last plane through colour_store.
// The bytes of a row's last dword beyond ow (padding) are computed like pixels and never stored to the canvas.  A pixel's taps are
// clamped to 0 .. ow - 1, so no pixel reads padding; only the lanes' work on the padding bytes themselves may read padding — of
// the first plane: bytes nobody wrote — inside the same dword, and what they make of it is padding again.
__device__ inline uint32_t blur_dword_along(const uint8_t *row, int n, int x0, int r, uint32_t ww, uint32_t fw) {
    uint32_t s = blur_window(row, 1, n, x0, r), out = 0;
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        if (j) s += (uint32_t)row[min(x + r, n - 1)] - (uint32_t)row[max(x - 1 - r, 0)];
        out |= blur_byte(ww, fw, s, (uint32_t)row[max(x - r - 1, 0)] + row[min(x + r + 1, n - 1)]) << (8 * j);
    }
    return out;
}
__device__ inline uint32_t blur_dword_across(const uint32_t *col, int pitch, int n, int y, int r, uint32_t ww, uint32_t fw) {
    const int lo = max(y - r, 0), hi = min(y + r, n - 1);
    const uint32_t cl = (uint32_t)(lo - (y - r)), cr = (uint32_t)(y + r - hi), top = col[0], bot = col[(n - 1) * pitch];
    uint32_t s[4];
    for (int j = 0; j < 4; ++j) s[j] = cl * (top >> (8 * j) & 0xFFu) + cr * (bot >> (8 * j) & 0xFFu);
    for (int i = lo; i <= hi; ++i) {
        const uint32_t w = col[i * pitch];
        for (int j = 0; j < 4; ++j) s[j] += w >> (8 * j) & 0xFFu;
    }
    const uint32_t fa = col[max(y - r - 1, 0) * pitch], fb = col[min(y + r + 1, n - 1) * pitch];
    uint32_t out = 0;
    for (int j = 0; j < 4; ++j) out |= blur_byte(ww, fw, s[j], (fa >> (8 * j) & 0xFFu) + (fb >> (8 * j) & 0xFFu)) << (8 * j);
    return out;
}

template <int C>
__global__ __launch_bounds__(1024) void k_colour_blur(const ColourArgs a, const ColourBlurArgs b, const int step) {
    extern __shared__ uint32_t blur_planes[];
    const int64_t wg = workgroup_index();
    const int first = b.first[step], n_list = b.first[step + 1] - first;
    if (wg >= (int64_t)n_list * C) return;
    const int64_t k = b.list[first + (int)(wg / C)];
    const int c = (int)(wg % C), t = threadIdx.x, nt = blockDim.x;
    const DevColourOutput &o = a.outputs[k];
    const int r = o.ivalue[step], passes = colour_blur_passes(o.kind[step]);
    const uint32_t ww = b.weights[(k * 4 + step) * 2], fw = b.weights[(k * 4 + step) * 2 + 1];
    const int ow = a.ow, oh = a.oh, pitch = (ow + 3) >> 2, dwords = pitch * oh, npix = ow * oh;       // (npix <= kBlurLdsMax / 2)
    const bool rowmajor = (a.layout & 1) != 0;
    const int64_t ps = a.layout >= 2 ? 1 : C, cs = a.layout >= 2 ? npix : 1;
    uint32_t *cur = blur_planes, *next = blur_planes + dwords;
    const unsigned char *src = a.canvas[step & 1] + k * npix * C + c * cs;
    for (int p = t; p < npix; p += nt) {
        const int x = rowmajor ? p % ow : p / oh, y = rowmajor ? p / ow : p % oh;
        reinterpret_cast<uint8_t *>(cur)[y * pitch * 4 + x] = src[p * ps];
    }
    __syncthreads();
    for (int pass = 0; pass < 2 * passes; ++pass) {
        for (int i = t; i < dwords; i += nt) {
            const int y = i / pitch, xd = i - y * pitch;
            next[i] = pass < passes ? blur_dword_along(reinterpret_cast<const uint8_t *>(cur + y * pitch), ow, xd * 4, r, ww, fw)
                                    : blur_dword_across(cur + xd, pitch, oh, y, r, ww, fw);
        }
        __syncthreads();
        uint32_t *swap = cur; cur = next; next = swap;
    }
    for (int p = t; p < npix; p += nt) {
        const int x = rowmajor ? p % ow : p / oh, y = rowmajor ? p / ow : p % oh;
        const unsigned v = reinterpret_cast<const uint8_t *>(cur)[y * pitch * 4 + x];
        colour_store<C, 1>(a, o, step, k, p, x, y, c, &v);
    }
}

// The pass launch, for canvases whose two planes LDS does not hold: one thread per pixel of the step's blur outputs, pass `pass` of
// the output's 2 or 6 — canvas A = canvas[step & 1] -> scratch T -> A -> ... -> T -> colour_store (every chain of passes is even, so
// its last pass reads T).  A's part of a blur output is free within the step: no other launch of the step reads it.
template <int C>
__global__ __launch_bounds__(256) void k_colour_blur_pass(const ColourArgs a, const ColourBlurArgs b, const int step, const int pass) {
    const int64_t npix = (int64_t)a.ow * a.oh, per_output = (npix + 255) / 256;
    const int64_t wg = workgroup_index();
    const int first = b.first[step], n_list = b.first[step + 1] - first;
    if (wg >= n_list * per_output) return;
    const int64_t k = b.list[first + (int)(wg / per_output)], p = (wg % per_output) * 256 + threadIdx.x;
    if (p >= npix) return;
    const DevColourOutput &o = a.outputs[k];
    const int passes = colour_blur_passes(o.kind[step]);
    if (pass >= 2 * passes) return;
    const bool rowmajor = (a.layout & 1) != 0;
    const int x = rowmajor ? (int)(p % a.ow) : (int)(p / a.oh), y = rowmajor ? (int)(p / a.ow) : (int)(p % a.oh);
    const int64_t ps = a.layout >= 2 ? 1 : C, cs = a.layout >= 2 ? npix : 1;
    const int64_t sx = rowmajor ? 1 : a.oh, sy = rowmajor ? a.ow : 1;
    const bool along = pass < passes;
    const unsigned char *line = (pass & 1 ? b.scratch : a.canvas[step & 1]) + k * npix * C + (along ? p - x * sx : p - y * sy) * ps;
    unsigned v[C];
    for (int c = 0; c < C; ++c)
        v[c] = blur_pixel(line + c * cs, (along ? sx : sy) * ps, along ? a.ow : a.oh, along ? x : y, o.ivalue[step], b.weights[(k * 4 + step) * 2], b.weights[(k * 4 + step) * 2 + 1]);
    if (pass + 1 < 2 * passes) {
        unsigned char *dst = (pass & 1 ? a.canvas[step & 1] : b.scratch) + k * npix * C;
        for (int c = 0; c < C; ++c) dst[p * ps + c * cs] = (unsigned char)v[c];
        return;
    }
    colour_store<C, C>(a, o, step, k, p, x, y, 0, v);
}

dim3 grid_for(int64_t total) {
    const int64_t gx = std::min<int64_t>(total, kResizeGridX);
    return dim3((unsigned)gx, (unsigned)((total + gx - 1) / gx));
}

template <int C>
hipError_t launch_colour_t(hipStream_t stream, const ColourArgs &a, const ColourBlurArgs &b, const ColourHueArgs &h) {
    const int64_t npix = (int64_t)a.ow * a.oh;
    static OncePerDevice attr_once;
    attr_once.run([&] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_colour_blur<C>), hipFuncAttributeMaxDynamicSharedMemorySize, kBlurLdsMax);
    });
    for (int s = 0; s < a.steps; ++s) {
        const int n_list = a.hist_first[s + 1] - a.hist_first[s];
        if (n_list > 0) {
            if (hipError_t e = hipMemsetAsync(a.hist, 0, (size_t)a.n_outputs * 1024 * sizeof(uint32_t), stream); e != hipSuccess) return e;
            const int64_t chunks = (npix + kColourHistPixels - 1) / kColourHistPixels;
            hipLaunchKernelGGL((k_colour_hist<C>), grid_for(n_list * chunks), dim3(256), 0, stream, a, s);
        }
        if (a.tables_at >> s & 1) hipLaunchKernelGGL((k_colour_tables<C>), grid_for(a.n_outputs), dim3(64), 0, stream, a, s);
        const int n_blur = b.first[s + 1] - b.first[s], n_hue = h.first[s + 1] - h.first[s];
        // (k_colour_apply reads a blur or hue output's pixel before it returns: a step whose outputs are ALL such goes without the launch)
        if (n_blur + n_hue < a.n_outputs) hipLaunchKernelGGL((k_colour_apply<C>), grid_for(a.n_outputs * ((npix + 255) / 256)), dim3(256), 0, stream, a, s);
        if (n_blur > 0 && b.lds) {
            const int dwords = b.lds / 8;
            hipLaunchKernelGGL((k_colour_blur<C>), grid_for((int64_t)n_blur * C), dim3((unsigned)std::min(1024, (dwords + 63) & ~63)), (size_t)b.lds, stream, a, b, s);
        } else if (n_blur > 0) {
            for (int pass = 0; pass < b.passes[s]; ++pass)
                hipLaunchKernelGGL((k_colour_blur_pass<C>), grid_for(n_blur * ((npix + 255) / 256)), dim3(256), 0, stream, a, b, s, pass);
        }
        if constexpr (C == 3)
            if (n_hue > 0) hipLaunchKernelGGL(k_colour_hue, grid_for(n_hue * (((npix + 3) / 4 + 255) / 256)), dim3(256), 0, stream, a, h, s);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the host twin of one op on a row-major interleaved image (out != src)
template <int C>
void colour_host_op(const uint8_t *src, int w, int h, const mj_colour_op &op, uint8_t *out) {
    const int64_t npix = (int64_t)w * h;
    const int kind = op.kind, iv = colour_ivalue(op);
    if (colour_is_blur(kind)) {
        const BlurPass b = colour_blur_pass(op);
        const int passes = colour_blur_passes(kind);
        std::vector<uint8_t> cur(src, src + npix * C), next((size_t)npix * C);
        for (int pass = 0; pass < 2 * passes; ++pass) {
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x)
                    for (int c = 0; c < C; ++c)
                        next[(size_t)(((int64_t)y * w + x) * C + c)] = (uint8_t)(pass < passes ? blur_pixel(cur.data() + (int64_t)y * w * C + c, C, w, x, b.r, b.ww, b.fw)
                                                                                             : blur_pixel(cur.data() + (int64_t)x * C + c, (int64_t)w * C, h, y, b.r, b.ww, b.fw));
            cur.swap(next);
        }
        memcpy(out, cur.data(), (size_t)npix * C);
        return;
    }
    if (kind == MJ_COLOUR_ADJUST_HUE && C == 3) {
        static const HueTables tables = colour_hue_tables();
        for (int64_t p = 0; p < npix; ++p) {
            unsigned r[3];
            colour_hue(src[p * 3], src[p * 3 + 1], src[p * 3 + 2], iv, tables.f, tables.fs, tables.sextant, r);
            for (int c = 0; c < 3; ++c) out[p * 3 + c] = (uint8_t)r[c];
        }
        return;
    }
    if (colour_is_table(kind)) {
        std::vector<uint32_t> hist(4 * 256, 0);
        std::vector<unsigned long long> prefix(4 * 256, 0);
        ColourStats stats[4] = {};
        unsigned long long wsums[4] = {};
        const int L = C == 3 ? 3 : 0;
        if (colour_needs_hist(kind)) {
            for (int64_t p = 0; p < npix; ++p) {
                for (int c = 0; c < C; ++c) ++hist[(size_t)(c * 256 + src[p * C + c])];
                if (C == 3) ++hist[(size_t)(768 + mode_luma(src[p * 3], src[p * 3 + 1], src[p * 3 + 2]))];
            }
            for (int b = 0; b < 4; ++b) colour_scan(hist.data() + b * 256, prefix.data() + b * 256, stats[b], wsums[b]);
        }
        uint8_t tab[C][256];
        for (int c = 0; c < C; ++c) {
            ColourStats st = stats[c];
            st.mean = colour_mean(wsums[L], stats[L].total);
            for (int i = 0; i < 256; ++i) tab[c][i] = (uint8_t)colour_table_entry(kind, op.value, iv, i, st, prefix[(size_t)(c * 256 + i)]);
        }
        for (int64_t p = 0; p < npix; ++p)
            for (int c = 0; c < C; ++c) out[p * C + c] = tab[c][src[p * C + c]];
        return;
    }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int64_t p = (int64_t)y * w + x;
            for (int c = 0; c < C; ++c) out[p * C + c] = src[p * C + c];
            if (kind == MJ_COLOUR_COLOR && C == 3) {
                const int l = (int)mode_luma(src[p * 3], src[p * 3 + 1], src[p * 3 + 2]);
                for (int c = 0; c < C; ++c) out[p * C + c] = (uint8_t)colour_blend(l, src[p * C + c], op.value);
            } else if (kind == MJ_COLOUR_SHARPNESS && x > 0 && y > 0 && x < w - 1 && y < h - 1) {
                for (int c = 0; c < C; ++c) {
                    float nb[3][3];
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) nb[dy + 1][dx + 1] = (float)src[(p + dx + (int64_t)dy * w) * C + c];
                    out[p * C + c] = (uint8_t)colour_blend((int)colour_smooth(nb), src[p * C + c], op.value);
                }
            }
        }
}

}  // namespace

const char *colour_fault(const mj_colour_chain &c) {
    if (c.n < 0 || c.n > MJ_COLOUR_MAX_OPS) return "a chain has 0..MJ_COLOUR_MAX_OPS ops";
    for (int s = 0; s < c.n; ++s) {
        const mj_colour_op &op = c.op[s];
        if (op.kind < MJ_COLOUR_BRIGHTNESS || (op.kind > MJ_COLOUR_BOX_BLUR && op.kind != MJ_COLOUR_ADJUST_HUE)) return "an op's kind is none of MJ_COLOUR_*";
        const bool valued = op.kind <= MJ_COLOUR_SOLARIZE || colour_is_blur(op.kind) || op.kind == MJ_COLOUR_ADJUST_HUE;
        if (valued && !std::isfinite(op.value)) return "an op's value is not finite";
        if (colour_is_blur(op.kind) && !(op.value >= 0.0f && op.value <= kBlurMaxRadius)) return "a blur takes a radius of 0..1024";
        if (op.kind == MJ_COLOUR_ADJUST_HUE && !(op.value >= -0.5f && op.value <= 0.5f)) return "adjust_hue takes a factor of -0.5..0.5";
        if (op.kind == MJ_COLOUR_POSTERIZE && !(op.value >= 1.0f && op.value <= 8.0f && op.value == floorf(op.value))) return "posterize takes 1..8 bits";
    }
    return nullptr;
}

int colour_ivalue(const mj_colour_op &op) {
    if (op.kind == MJ_COLOUR_POSTERIZE) return ~((1 << (8 - (int)op.value)) - 1) & 0xFF;
    if (op.kind == MJ_COLOUR_SOLARIZE) return (int)std::min(std::max(ceilf(op.value), 0.0f), 256.0f);
    if (colour_is_blur(op.kind)) return colour_blur_pass(op).r;
    // torchvision's np.array(f * 255).astype(np.uint8): the double product truncated toward zero, then wrapped
    if (op.kind == MJ_COLOUR_ADJUST_HUE) return (int)((double)op.value * 255) & 255;
    return 0;
}

// Pillow's BoxBlur.c: the box radius of a Gaussian's three passes (_gaussian_blur_radius: float32, the square root and the floor
// in double) and the weights of a pass (ImagingLineBoxBlur8), every operation rounded on its own
BlurPass colour_blur_pass(const mj_colour_op &op) {
    float fr = op.value;
    if (op.kind == MJ_COLOUR_GAUSSIAN_BLUR) {
        const float sigma2 = op.value * op.value / 3;
        const float L = (float)sqrt(12.0 * sigma2 + 1.0);
        const float l = (float)floor((L - 1.0) / 2.0);
        float a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
        a /= 6 * (sigma2 - (l + 1) * (l + 1));
        fr = l + a;
    }
    BlurPass b;
    b.r = (int)fr;
    b.ww = (uint32_t)((float)(1 << 24) / (fr * 2 + 1));
    b.fw = ((1u << 24) - (uint32_t)(b.r * 2 + 1) * b.ww) / 2;
    return b;
}

hipError_t launch_colour(hipStream_t stream, const ColourArgs &a, const ColourBlurArgs &b, const ColourHueArgs &h) {
    if (a.n_outputs <= 0 || a.steps <= 0) return hipSuccess;
    return a.C == 3 ? launch_colour_t<3>(stream, a, b, h) : launch_colour_t<1>(stream, a, b, h);
}

}  // namespace mj

extern "C" {

int mj_host_colour_ops(const uint8_t *src, int32_t w, int32_t h, int32_t ncomp, const mj_colour_chain *chain, uint8_t *out) {
    if (!src || !out || !chain || w < 1 || h < 1 || (ncomp != 1 && ncomp != 3) || mj::colour_fault(*chain)) return MJ_ERR_INVALID;
    const size_t bytes = (size_t)w * h * ncomp;
    std::vector<uint8_t> cur(src, src + bytes), next(bytes);
    for (int s = 0; s < chain->n; ++s) {
        if (ncomp == 3) mj::colour_host_op<3>(cur.data(), w, h, chain->op[s], next.data());
        else mj::colour_host_op<1>(cur.data(), w, h, chain->op[s], next.data());
        cur.swap(next);
    }
    memcpy(out, cur.data(), bytes);
    return MJ_OK;
}

}  // extern "C"
