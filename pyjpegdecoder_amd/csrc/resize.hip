// Decode to a fixed size: the batch's decoded pixels (whole images or windows, as stage 2 packed them) resized to one
// out_width x out_height, all images in ONE launch, into one dense output.
//
// The arithmetic is Pillow's Image.resize(size, filter) on 8-bit data (tools/resize_model.py restates it) for BILINEAR — the
// default — BOX, HAMMING, BICUBIC and LANCZOS (mj_plan_request.filter): per axis a
// table of integer taps — the filter's weights in doubles, support growing with the scale when shrinking, normalised,
// rounded to 22 bits: build_resize_axis, host — and per pixel clip8((2^21 + sum taps * in) >> 22), signed and clamped at both
// ends where the filter's taps go below zero (Tap).  Two passes with a uint8
// intermediate image: along the width first, then along the height.  The order and the intermediate rounding are part of the
// result.  (An axis that does not change goes through the same code: its table is one tap of 2^22, which is the identity.)
//
// A workgroup takes one tile of one image's output.  It runs the width pass for the source rows the tile needs into LDS —
// that IS the intermediate image — then the height pass out of LDS, and stores finished output.  Source bytes are read 16 per
// lane along the contiguous axis of the source, which differs with the layout:
//   row-major source (H, W, C): the width pass runs ALONG the contiguous axis.  A wavefront stages one source row segment in
//     LDS (aligned 16-byte loads) and gathers its taps from there; the height pass then runs across the rows of T.
//   x-major source (W, H, C):   the width pass runs ACROSS the contiguous axis.  A lane holds 16 consecutive bytes (y, c) of a
//     column and accumulates the taps' columns straight from global memory (16-byte loads at any alignment: columns start
//     where they start); the height pass then gathers along the rows of T.
// Planar plans read the same interleaved source (stage 2 writes it; the plane separation of a plain planar plan is skipped)
// and only store elsewhere.
//
// Model-ready output (mj_plan_request.output): the height pass ends in a byte v of component c, and what it stores is a
// pure function of (c, v) — torchvision's Normalize(mean, std)(to_tensor(img)) in float32, operation by operation, then
// rounded to nearest even for the 16-bit types (tools/normalize_model.py).  The host evaluates it for the 256 x C pairs
// (build_normalize_table) and the kernels' 2- and 4-byte instances store lut[c][v] out of LDS: exact by construction, no
// float arithmetic on the device.  float16 and bfloat16 share the 2-byte instance (the table holds the bits).  Mirror is a
// per-image flag (ResizeArgs::mirror) of the mirror instances: the element goes to column out_width - 1 - x.  A lane still stores one element
// and consecutive lanes consecutive elements of the output's contiguous axis, so a wavefront's store is one run of 64, 128
// or 256 bytes (descending for a mirrored image of a row-major layout); the plain uint8 instances are the code they were.
//
// Output colour mode (mj_plan_request.mode with a size): the k_resize_*_mode instances, whose source has CS components and whose
// output CO — greyscale files into three components (Pillow's convert("RGB")) and colour files into one (convert("L"),
// mode_luma of the decoded RGB bytes).  The conversion comes first, as in img.convert(mode).resize(size): colour to L where the
// source is read, before any tap (the staged row in LDS; 16 pixels = 48 bytes per lane and tap in registers), so both passes and
// T run on ONE component either way.  Grey to RGB finishes every pixel's sum once into a tile of bytes in LDS and the store
// loop — one element per lane, consecutive lanes consecutive elements, as above — looks up lut[c][byte] for c = 0..2.  They
// are instances in the oriented style only (the per-image byte holds the flips and the mirror flag; all zero for a plain plan).
//
// Aspect-preserving sizing (mj_plan_request.places): the output is a canvas, every image is resized to a size of its own and
// placed at an offset on it; elements it does not cover hold a fill byte, which takes the output's path like any other.  The tap
// tables are built in the canvas's coordinates — an entry outside the image has no taps and keeps the bound of the nearest entry inside
// as its first index — so the placed instances of the four kernels (the ones with a trailing fill argument: fill_arg) compute canvas
// elements only: a tile the image does not reach stores fill and returns before any staging, a tile it reaches runs the width pass
// over the covered columns and rows alone.  With windows, plan creation shrinks every window to the source range the canvas needs.
// This file: the tables' and the output table's arithmetic (host), the kernels, and launch_resize, the one place that maps a plan
// to an instance.  Plan creation (a request with a size: tables, tile, LDS layout, the placed source ranges) is resize_plan.hip.
#include <math.h>

#include <type_traits>

#include "plan.h"

namespace mj {

// ---- host: tap tables -----------------------------------------------------------------------------------------------
// xmin[out], count[out], taps[out][ksize] (zeros behind count); the formulas and their evaluation order are Pillow's
// (precompute_coeffs + normalize_coeffs_8bpc with the filter's function and support).  Compiled with -ffp-contract=off like
// everything here; sin and cos are the host's libm, as they are Pillow's.
namespace {

const double kPi = 3.14159265358979323846;

double f_bilinear(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
double f_box(double x) { return x > -0.5 && x <= 0.5 ? 1.0 : 0.0; }
double f_hamming(double x) {
    if (x < 0.0) x = -x;
    if (x == 0.0) return 1.0;
    if (x >= 1.0) return 0.0;
    x = x * kPi;
    return sin(x) / x * (0.54f + 0.46f * cos(x));      // (the two constants are float literals in Pillow: part of the result)
}
double f_bicubic(double x) {       // a = -0.5, Pillow's Horner form
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * -0.5;
    return 0.0;
}
double f_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * kPi;
    return sin(x) / x;
}
double f_lanczos(double x) { return -3.0 <= x && x < 3.0 ? f_sinc(x) * f_sinc(x / 3) : 0.0; }

struct FilterDef { double support; double (*f)(double); };
// (indexed by MJ_FILTER_*)
const FilterDef kFilters[] = {{1.0, f_bilinear}, {0.5, f_box}, {1.0, f_hamming}, {2.0, f_bicubic}, {3.0, f_lanczos}};

}  // namespace

bool resize_filter_known(int filter) { return filter >= 0 && filter < (int)(sizeof(kFilters) / sizeof(kFilters[0])); }
// taps below zero (side lobes): the kernels' signed instances
bool resize_filter_signed(int filter) { return filter == MJ_FILTER_BICUBIC || filter == MJ_FILTER_LANCZOS; }

// (the scale of an axis: the part of the source the table resamples — box, two 32-bit floats whose difference is a float's —
// over the entries it makes of it; NULL: the whole axis)
static double axis_scale(int in_size, int out_size, const float *box) {
    return box ? (double)(box[1] - box[0]) / out_size : (double)in_size / (double)out_size;
}

int resize_axis_ksize(int in_size, int out_size, int filter, const float *box) {
    const double scale = axis_scale(in_size, out_size, box);
    const double support = kFilters[filter].support * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}

void build_resize_axis(int in_size, int out_size, int32_t *xmin, int32_t *count, int32_t *taps, int taps_stride, int filter, const float *box) {
    const FilterDef &F = kFilters[filter];
    const double scale = axis_scale(in_size, out_size, box), in0 = box ? (double)box[0] : 0.0;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = F.support * filterscale, ss = 1.0 / filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    std::vector<double> w((size_t)ksize + 2);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = in0 + (xx + 0.5) * scale;      // (in0 0: the product itself)
        int lo = (int)(center - support + 0.5);
        if (lo < 0) lo = 0;
        int hi = (int)(center + support + 0.5);
        if (hi > in_size) hi = in_size;
        int n = hi - lo;
        if (n > ksize) n = ksize;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            w[x] = F.f(((double)(x + lo) - center + 0.5) * ss);
            ww += w[x];
        }
        xmin[xx] = lo;
        count[xx] = n;
        for (int x = 0; x < taps_stride; ++x) {
            double v = x < n ? w[x] : 0.0;
            if (x < n && ww != 0.0) v /= ww;
            // (rounded away from zero, as normalize_coeffs_8bpc does)
            taps[(size_t)xx * taps_stride + x] = x >= n ? 0 : v < 0.0 ? (int32_t)(v * (double)(1 << 22) - 0.5) : (int32_t)(v * (double)(1 << 22) + 0.5);
        }
    }
}

// ---- device ---------------------------------------------------------------------------------------------------------
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct AxisTab {
    const int32_t *lo, *cnt, *k;
    int ks;
    __device__ AxisTab(const int32_t *t, int out) : lo(t + 1), cnt(t + 1 + out), k(t + 1 + 2 * out), ks(t[0]) {}
};

// where output element (ox, oy, c) of an image goes: a.layout is the plan's MJ_LAYOUT_*
__device__ __forceinline__ int64_t out_index(const ResizeArgs &a, int C, int ox, int oy, int c) {
    switch (a.layout) {
        case 0: return ((int64_t)ox * a.oh + oy) * C + c;          // (ow, oh, C)
        case 1: return ((int64_t)oy * a.ow + ox) * C + c;          // (oh, ow, C)
        case 2: return ((int64_t)c * a.ow + ox) * a.oh + oy;       // (C, ow, oh)
        default: return ((int64_t)c * a.oh + oy) * a.ow + ox;      // (C, oh, ow)
    }
}

__device__ __forceinline__ unsigned clip8(unsigned acc) {
    const unsigned v = acc >> 22;
    return v > 255u ? 255u : v;
}

// One output byte's sum.  Tap<false>: every tap is >= 0 (bilinear, box, hamming) — unsigned sums, the unsigned 24-bit multiply,
// a clamp at the top: the instances that were there before the other filters, the code they were.  Tap<true>: taps with negative
// side lobes (bicubic, Lanczos) — int sums, the signed 24-bit multiply (plan creation holds every |tap| below 2^23 and every
// 2^21 + 255 * sum |tap| below 2^31), an arithmetic shift and a clamp at both ends.
template <bool SGN> struct Tap {
    typedef unsigned acc_t;
    static __device__ __forceinline__ unsigned mul(int32_t k, unsigned v) { return __umul24((unsigned)k, v); }
    static __device__ __forceinline__ unsigned clip(unsigned acc) { return clip8(acc); }
};
template <> struct Tap<true> {
    typedef int acc_t;
    static __device__ __forceinline__ int mul(int32_t k, unsigned v) { return __mul24(k, (int)v); }
    // (the lower clamp in front of the shift, which is then a logical one: written as clamp(acc >> 22, 0, 255) the compiler packs
    // pairs of these with v_ashr_pk_u8_i32, and what came back from the chip was not clamped at 0)
    static __device__ __forceinline__ unsigned clip(int acc) { return min((unsigned)max(acc, 0) >> 22, 255u); }
};

// the element a finished byte v of component c is stored as: the byte, or its entry of the workgroup's table
template <typename OutT>
__device__ __forceinline__ OutT out_value(const OutT *lut, int c, unsigned v) {
    if constexpr (sizeof(OutT) == 1) return (OutT)v;
    else return lut[c * 256 + v];
}

// every workgroup's copy of the plan's table (256 x C elements behind the kernel's other LDS); the caller's barrier follows
template <int C, typename OutT>
__device__ __forceinline__ const OutT *stage_lut(const ResizeArgs &a, unsigned char *smem, int tid) {
    if constexpr (sizeof(OutT) == 1) return nullptr;
    else {
        OutT *lut = reinterpret_cast<OutT *>(smem + a.lut_off);
        const OutT *g = static_cast<const OutT *>(a.lut);
        for (int i = tid; i < 256 * C; i += 256) lut[i] = g[i];
        return lut;
    }
}

// ---- placed plans (mj_plan_request.places): `fill` holds the canvas's fill byte of component c in bits 8c..8c+7
__device__ __forceinline__ unsigned fill_byte(unsigned fill, int c) { return (fill >> (8 * c)) & 255u; }
// The placed instances of a kernel are the ones with a trailing kernel argument (`Fill... fill`, one unsigned): the
// oriented-style instance over canvas tables — entries outside the image have no taps and keep the bound of the nearest entry
// inside as their first index, so a tile's span covers only what the image needs and the width pass runs over that alone — plus
// two things under PLACED: a tile the image does not reach stores fill and returns, and an element without taps on either axis
// stores its fill byte.  ResizeArgs and every other instance's signature stay, and the discarded branches leave those the functions they were.
template <typename... Fill> __device__ __forceinline__ unsigned fill_arg(const Fill... fill) { return (0u | ... | fill); }

// A tile no pixel of which the image covers: every element is the fill element, stored in the order the height pass stores
// (XM: along the columns) — before any staging, so the table entry comes from global memory.
template <int C, typename OutT, bool XM>
__device__ __forceinline__ void fill_tile(const ResizeArgs &a, const DevResizeImage &im, int img, unsigned fill, int ox0, int oy0, int ncols, int orows) {
    OutT *dst = reinterpret_cast<OutT *>(a.dst + im.dst_off);
    const OutT *lut = static_cast<const OutT *>(a.lut);
    const unsigned turn = a.mirror[img];
    const bool planar = a.layout >= 2 && C > 1;
    const int npix = orows * ncols, fast = XM ? orows : ncols;
    for (int i = threadIdx.x; i < npix * C; i += 256) {
        int pix, c;
        if (planar) { c = i / npix; pix = i - c * npix; } else { pix = i / C; c = i - pix * C; }
        const int slow = pix / fast, f = pix - slow * fast;
        const int ox = ox0 + (XM ? slow : f), oy = oy0 + (XM ? f : slow);
        dst[out_index(a, C, (turn & 1) ? a.ow - 1 - ox : ox, (turn & 2) ? a.oh - 1 - oy : oy, c)] = out_value<OutT>(lut, c, fill_byte(fill, c));
    }
}

// Row-major source.  LDS: T [t_rows][t_pitch] | per output column of the tile: first source column (relative), taps, the
// taps themselves [tc][ksx] | one staging row per wavefront | the output table (2- and 4-byte elements).
template <int C, typename OutT = unsigned char, bool MIRROR = false, bool ORIENT = false, bool SGN = false, typename... Fill>
__global__ __launch_bounds__(256) void k_resize_rowmajor(const ResizeArgs a, Fill... fill) {
    constexpr bool PLACED = sizeof...(Fill) == 1;
    static_assert(sizeof...(Fill) <= 1 && (!PLACED || (ORIENT && !MIRROR)), "placed instances: one fill word, the oriented style");
    typedef typename Tap<SGN>::acc_t acc_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tiles = a.tiles_x * a.tiles_y;
    const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;      // (launch_resize: the grid's tail is idle)
    if (wg >= (int64_t)a.n_images * tiles) return;
    const int img = (int)(wg / tiles), t = (int)(wg - (int64_t)img * tiles);
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const DevResizeImage im = a.images[img];
    const int ox0 = tx * a.tc, ox1 = min(ox0 + a.tc, a.ow), oy0 = ty * a.tr, oy1 = min(oy0 + a.tr, a.oh);
    const AxisTab X(a.tabs + im.xtab, a.ow), Y(a.tabs + im.ytab, a.oh);
    const int xa = X.lo[ox0], xb = X.lo[ox1 - 1] + X.cnt[ox1 - 1];       // (both bounds grow with the output index)
    const int ya = Y.lo[oy0], yb = Y.lo[oy1 - 1] + Y.cnt[oy1 - 1];
    const int nrows = yb - ya, ncols = ox1 - ox0, ne = ncols * C;
    // (a tile the image does not reach: no source entries along an axis)
    if constexpr (PLACED) { if (xb == xa || yb == ya) { fill_tile<C, OutT, false>(a, im, img, fill_arg(fill...), ox0, oy0, ncols, oy1 - oy0); return; } }
    unsigned char *T = smem;
    int32_t *lx_lo = reinterpret_cast<int32_t *>(smem + a.tab_off), *lx_cnt = lx_lo + a.tc, *lx_k = lx_cnt + a.tc;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    unsigned char *stage = smem + a.stage_off + wave * a.stage_bytes;
    for (int i = tid; i < ncols; i += 256) { lx_lo[i] = (X.lo[ox0 + i] - xa) * C; lx_cnt[i] = X.cnt[ox0 + i]; }
    for (int i = tid; i < ncols * X.ks; i += 256) lx_k[i] = X.k[(int64_t)ox0 * X.ks + i];
    const OutT *lut = stage_lut<C, OutT>(a, smem, tid);
    __syncthreads();
    const unsigned char *src = a.src + im.src_off;
    const int seg = (xb - xa) * C;
    // width pass: every wavefront takes every fourth source row of the tile
    for (int r = wave; r < nrows; r += 4) {
        const unsigned char *row = src + ((int64_t)(ya + r) * im.w + xa) * C;
        const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 15);
        const u32x4 *p = reinterpret_cast<const u32x4 *>(row - mis);
        const int n16 = (mis + seg + 15) >> 4;
        for (int j = lane; j < n16; j += 64) reinterpret_cast<u32x4 *>(stage)[j] = p[j];
        // (the staging row is this wavefront's own: its lanes only have to see each other's LDS writes)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int e = lane; e < ne; e += 64) {
            const int oxl = e / C, c = e - oxl * C;
            const unsigned char *s = stage + mis + lx_lo[oxl] + c;
            const int32_t *k = lx_k + oxl * X.ks;
            const int n = lx_cnt[oxl];
            acc_t acc = (acc_t)1 << 21;
            for (int q = 0; q < n; ++q) acc += Tap<SGN>::mul(k[q], (unsigned)s[q * C]);
            T[r * a.t_pitch + e] = (unsigned char)Tap<SGN>::clip(acc);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();
    // height pass: consecutive lanes take consecutive elements of an output row (of a plane's row for planar plans)
    OutT *dst = reinterpret_cast<OutT *>(a.dst + im.dst_off);
    const bool flip = MIRROR && a.mirror[img] != 0;
    unsigned turn = 0;      // oriented plans: bit 0 = store at column ow - 1 - x, bit 1 = at row oh - 1 - y
    if constexpr (ORIENT) turn = a.mirror[img];
    const int orows = oy1 - oy0, total = orows * ne;
    const bool planar = a.layout >= 2 && C > 1;
    for (int i = tid; i < total; i += 256) {
        int oyl, oxl, c;
        if (planar) { c = i / (orows * ncols); const int rem = i - c * (orows * ncols); oyl = rem / ncols; oxl = rem - oyl * ncols; }
        else { oyl = i / ne; const int e = i - oyl * ne; oxl = e / C; c = e - oxl * C; }
        const int oy = oy0 + oyl;
        const int n = Y.cnt[oy];
        const int32_t *k = Y.k + (int64_t)oy * Y.ks;
        const unsigned char *s = T + (Y.lo[oy] - ya) * a.t_pitch + oxl * C + c;
        acc_t acc = (acc_t)1 << 21;
        for (int q = 0; q < n; ++q) acc += Tap<SGN>::mul(k[q], (unsigned)s[q * a.t_pitch]);
        const int ox = ox0 + oxl;
        // (placed: no taps on either axis — a canvas element the image does not cover)
        const unsigned v = (PLACED && (n == 0 || lx_cnt[oxl] == 0)) ? fill_byte(fill_arg(fill...), c) : Tap<SGN>::clip(acc);
        if constexpr (ORIENT) dst[out_index(a, C, (turn & 1) ? a.ow - 1 - ox : ox, (turn & 2) ? a.oh - 1 - oy : oy, c)] = out_value<OutT>(lut, c, v);
        else dst[out_index(a, C, flip ? a.ow - 1 - ox : ox, oy, c)] = out_value<OutT>(lut, c, v);
    }
}

// X-major source.  LDS: T [tc][t_pitch] (one row per output column: the bytes (y, c) of the source rows the tile needs,
// t_pitch a multiple of 16) | per output row of the tile: first source row (relative), taps, the taps themselves [tr][ksy] |
// the output table (2- and 4-byte elements).
template <int C, typename OutT = unsigned char, bool MIRROR = false, bool ORIENT = false, bool SGN = false, typename... Fill>
__global__ __launch_bounds__(256) void k_resize_xmajor(const ResizeArgs a, Fill... fill) {
    constexpr bool PLACED = sizeof...(Fill) == 1;
    static_assert(sizeof...(Fill) <= 1 && (!PLACED || (ORIENT && !MIRROR)), "placed instances: one fill word, the oriented style");
    typedef typename Tap<SGN>::acc_t acc_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tiles = a.tiles_x * a.tiles_y;
    const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;      // (launch_resize: the grid's tail is idle)
    if (wg >= (int64_t)a.n_images * tiles) return;
    const int img = (int)(wg / tiles), t = (int)(wg - (int64_t)img * tiles);
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const DevResizeImage im = a.images[img];
    const int ox0 = tx * a.tc, ox1 = min(ox0 + a.tc, a.ow), oy0 = ty * a.tr, oy1 = min(oy0 + a.tr, a.oh);
    const AxisTab X(a.tabs + im.xtab, a.ow), Y(a.tabs + im.ytab, a.oh);
    const int ya = Y.lo[oy0], yb = Y.lo[oy1 - 1] + Y.cnt[oy1 - 1];
    const int nrows = yb - ya, ncols = ox1 - ox0, orows = oy1 - oy0;
    // (a tile the image does not reach: no source entries along an axis)
    if constexpr (PLACED) { if (X.lo[ox1 - 1] + X.cnt[ox1 - 1] == X.lo[ox0] || yb == ya) { fill_tile<C, OutT, true>(a, im, img, fill_arg(fill...), ox0, oy0, ncols, orows); return; } }
    unsigned char *T = smem;
    int32_t *ly_lo = reinterpret_cast<int32_t *>(smem + a.tab_off), *ly_cnt = ly_lo + a.tr, *ly_k = ly_cnt + a.tr;
    const int tid = threadIdx.x;
    for (int i = tid; i < orows; i += 256) { ly_lo[i] = (Y.lo[oy0 + i] - ya) * C; ly_cnt[i] = Y.cnt[oy0 + i]; }
    for (int i = tid; i < orows * Y.ks; i += 256) ly_k[i] = Y.k[(int64_t)oy0 * Y.ks + i];
    const OutT *lut = stage_lut<C, OutT>(a, smem, tid);
    const unsigned char *src = a.src + im.src_off;
    // width pass: 16 consecutive bytes of a column per lane, the taps' columns one after the other.  (The last chunk of a
    // column reads up to 15 bytes behind the rows the tile needs — the next column's, or the buffer's padding — into T's
    // padding, which nothing reads.)
    const int nch = (nrows * C + 15) >> 4;
    const int64_t col = (int64_t)im.h * C;
    for (int i = tid; i < ncols * nch; i += 256) {
        const int oxl = i / nch, j = i - oxl * nch;
        const int ox = ox0 + oxl, n = X.cnt[ox];
        const int32_t *k = X.k + (int64_t)ox * X.ks;
        const unsigned char *p = src + ((int64_t)X.lo[ox] * im.h + ya) * C + 16 * j;
        acc_t acc[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) acc[b] = (acc_t)1 << 21;
        for (int q = 0; q < n; ++q, p += col) {
            u32x4 v;
            __builtin_memcpy(&v, p, 16);
            const int32_t kq = k[q];
#pragma unroll
            for (int b = 0; b < 16; ++b) acc[b] += Tap<SGN>::mul(kq, (v[b >> 2] >> (8 * (b & 3))) & 255u);
        }
        u32x4 o;
#pragma unroll
        for (int d = 0; d < 4; ++d)
            o[d] = Tap<SGN>::clip(acc[4 * d]) | Tap<SGN>::clip(acc[4 * d + 1]) << 8 | Tap<SGN>::clip(acc[4 * d + 2]) << 16 | Tap<SGN>::clip(acc[4 * d + 3]) << 24;
        *reinterpret_cast<u32x4 *>(T + oxl * a.t_pitch + 16 * j) = o;
    }
    __syncthreads();
    // height pass: consecutive lanes take consecutive elements of an output column (of a plane's column for planar plans)
    OutT *dst = reinterpret_cast<OutT *>(a.dst + im.dst_off);
    const bool flip = MIRROR && a.mirror[img] != 0;
    unsigned turn = 0;      // oriented plans: bit 0 = store at column ow - 1 - x, bit 1 = at row oh - 1 - y
    if constexpr (ORIENT) turn = a.mirror[img];
    const int ne = orows * C, total = ncols * ne;
    const bool planar = a.layout >= 2 && C > 1;
    for (int i = tid; i < total; i += 256) {
        int oyl, oxl, c;
        if (planar) { c = i / (orows * ncols); const int rem = i - c * (orows * ncols); oxl = rem / orows; oyl = rem - oxl * orows; }
        else { oxl = i / ne; const int e = i - oxl * ne; oyl = e / C; c = e - oyl * C; }
        const int n = ly_cnt[oyl];
        const int32_t *k = ly_k + oyl * Y.ks;
        const unsigned char *s = T + oxl * a.t_pitch + ly_lo[oyl] + c;
        acc_t acc = (acc_t)1 << 21;
        for (int q = 0; q < n; ++q) acc += Tap<SGN>::mul(k[q], (unsigned)s[q * C]);
        const int ox = ox0 + oxl;
        // (placed: no taps on either axis — a canvas element the image does not cover)
        const unsigned v = (PLACED && (n == 0 || X.cnt[ox] == 0)) ? fill_byte(fill_arg(fill...), c) : Tap<SGN>::clip(acc);
        if constexpr (ORIENT) dst[out_index(a, C, (turn & 1) ? a.ow - 1 - ox : ox, (turn & 2) ? a.oh - 1 - (oy0 + oyl) : oy0 + oyl, c)] = out_value<OutT>(lut, c, v);
        else dst[out_index(a, C, flip ? a.ow - 1 - ox : ox, oy0 + oyl, c)] = out_value<OutT>(lut, c, v);
    }
}

// ---- output colour mode: source components CS != output components CO (T, both passes and the tile geometry: one component)
// The end of the height pass.  CO == 1: the finished byte is the element.  CO == 3: every pixel's byte goes into the tile O in LDS
// once; after the barrier a lane stores one element (pixel, c), looked up in component c's table.
// XM: T is [column][t_pitch] and a tile is walked along its columns (the x-major kernel), else [row][t_pitch] along its rows.
// PLACED: xcnt[oxl] is the tap count of the tile's column oxl — 0 there, or on the height axis, marks an element the image does
// not cover, stored as the fill byte of its component (`fill`: fill_byte).
template <int CO, typename OutT, bool SGN, bool XM, bool PLACED>
__device__ __forceinline__ void mode_height_pass(const ResizeArgs &a, const DevResizeImage &im, int img, const unsigned char *T, unsigned char *O,
                                                 const OutT *lut, const int32_t *lo, const int32_t *cnt, const int32_t *k_all, int ks, int ya, int ox0,
                                                 int oy0, int ncols, int orows, int tid, const int32_t *xcnt, unsigned fill) {
    typedef typename Tap<SGN>::acc_t acc_t;
    OutT *dst = reinterpret_cast<OutT *>(a.dst + im.dst_off);
    const unsigned turn = a.mirror[img];      // bit 0 = store at column ow - 1 - x, bit 1 = at row oh - 1 - y
    const int npix = orows * ncols;
    for (int i = tid; i < npix; i += 256) {
        int oyl, oxl;
        if (XM) { oxl = i / orows; oyl = i - oxl * orows; } else { oyl = i / ncols; oxl = i - oyl * ncols; }
        // (lo / cnt / k_all: the height axis — the tile's copy in LDS, relative to ya (x-major), or the image's table (row-major))
        const int n = XM ? cnt[oyl] : cnt[oy0 + oyl];
        const int32_t *k = XM ? k_all + oyl * ks : k_all + (int64_t)(oy0 + oyl) * ks;
        const unsigned char *s = XM ? T + oxl * a.t_pitch + lo[oyl] : T + (lo[oy0 + oyl] - ya) * a.t_pitch + oxl;
        const int step = XM ? 1 : a.t_pitch;
        acc_t acc = (acc_t)1 << 21;
        for (int q = 0; q < n; ++q) acc += Tap<SGN>::mul(k[q], (unsigned)s[q * step]);
        unsigned v = Tap<SGN>::clip(acc);
        if constexpr (PLACED && CO == 1) { if (n == 0 || xcnt[oxl] == 0) v = fill_byte(fill, 0); }
        if constexpr (CO == 1) {
            const int ox = ox0 + oxl, oy = oy0 + oyl;
            dst[out_index(a, 1, (turn & 1) ? a.ow - 1 - ox : ox, (turn & 2) ? a.oh - 1 - oy : oy, 0)] = out_value<OutT>(lut, 0, v);
        } else O[i] = (unsigned char)v;
    }
    if constexpr (CO > 1) {
        __syncthreads();
        const bool planar = a.layout >= 2;
        const int fast = XM ? orows : ncols;      // pixels along the direction the tile is walked in
        for (int i = tid; i < npix * CO; i += 256) {
            int pix, c;
            if (planar) { c = i / npix; pix = i - c * npix; } else { pix = i / CO; c = i - pix * CO; }
            const int slow = pix / fast, f = pix - slow * fast;
            const int ox = ox0 + (XM ? slow : f), oy = oy0 + (XM ? f : slow);
            unsigned v = (unsigned)O[pix];
            if constexpr (PLACED) { if ((XM ? cnt[f] : cnt[oy]) == 0 || xcnt[XM ? slow : f] == 0) v = fill_byte(fill, c); }
            dst[out_index(a, CO, (turn & 1) ? a.ow - 1 - ox : ox, (turn & 2) ? a.oh - 1 - oy : oy, c)] = out_value<OutT>(lut, c, v);
        }
    }
}

// where the tile O lies: behind the output table
template <int CO, typename OutT>
__device__ __forceinline__ unsigned char *mode_tile(const ResizeArgs &a, unsigned char *smem) {
    return smem + a.lut_off + (sizeof(OutT) > 1 ? 256 * CO * (int)sizeof(OutT) : 0);
}

// Row-major source.  LDS as k_resize_rowmajor's with T in one component; a colour source's staging row is 3/4 of stage_bytes and
// the row's L bytes — converted there by the wavefront that staged it — take the last quarter.
template <int CS, int CO, typename OutT, bool SGN, typename... Fill>
__global__ __launch_bounds__(256) void k_resize_rowmajor_mode(const ResizeArgs a, Fill... fill) {
    constexpr bool PLACED = sizeof...(Fill) == 1;
    static_assert(sizeof...(Fill) <= 1, "placed instances: one fill word");
    typedef typename Tap<SGN>::acc_t acc_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tiles = a.tiles_x * a.tiles_y;
    const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;      // (launch_resize: the grid's tail is idle)
    if (wg >= (int64_t)a.n_images * tiles) return;
    const int img = (int)(wg / tiles), t = (int)(wg - (int64_t)img * tiles);
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const DevResizeImage im = a.images[img];
    const int ox0 = tx * a.tc, ox1 = min(ox0 + a.tc, a.ow), oy0 = ty * a.tr, oy1 = min(oy0 + a.tr, a.oh);
    const AxisTab X(a.tabs + im.xtab, a.ow), Y(a.tabs + im.ytab, a.oh);
    const int xa = X.lo[ox0], xb = X.lo[ox1 - 1] + X.cnt[ox1 - 1];
    const int ya = Y.lo[oy0], yb = Y.lo[oy1 - 1] + Y.cnt[oy1 - 1];
    const int nrows = yb - ya, ncols = ox1 - ox0, npx = xb - xa;
    if constexpr (PLACED) { if (xb == xa || yb == ya) { fill_tile<CO, OutT, false>(a, im, img, fill_arg(fill...), ox0, oy0, ncols, oy1 - oy0); return; } }
    unsigned char *T = smem;
    int32_t *lx_lo = reinterpret_cast<int32_t *>(smem + a.tab_off), *lx_cnt = lx_lo + a.tc, *lx_k = lx_cnt + a.tc;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    unsigned char *stage = smem + a.stage_off + wave * a.stage_bytes;
    for (int i = tid; i < ncols; i += 256) { lx_lo[i] = X.lo[ox0 + i] - xa; lx_cnt[i] = X.cnt[ox0 + i]; }
    for (int i = tid; i < ncols * X.ks; i += 256) lx_k[i] = X.k[(int64_t)ox0 * X.ks + i];
    const OutT *lut = stage_lut<CO, OutT>(a, smem, tid);
    __syncthreads();
    const unsigned char *src = a.src + im.src_off;
    const int seg = npx * CS;
    for (int r = wave; r < nrows; r += 4) {
        const unsigned char *row = src + ((int64_t)(ya + r) * im.w + xa) * CS;
        const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 15);
        const u32x4 *p = reinterpret_cast<const u32x4 *>(row - mis);
        const int n16 = (mis + seg + 15) >> 4;
        for (int j = lane; j < n16; j += 64) reinterpret_cast<u32x4 *>(stage)[j] = p[j];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const unsigned char *g = stage + mis;
        if constexpr (CS == 3) {
            // the staged row to L, pixel by pixel, before any tap sees it
            unsigned char *grey = stage + 3 * (a.stage_bytes >> 2);
            for (int x = lane; x < npx; x += 64) {
                const unsigned char *s = stage + mis + 3 * x;
                grey[x] = (unsigned char)mode_luma(s[0], s[1], s[2]);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            g = grey;
        }
        for (int e = lane; e < ncols; e += 64) {
            const unsigned char *s = g + lx_lo[e];
            const int32_t *k = lx_k + e * X.ks;
            const int n = lx_cnt[e];
            acc_t acc = (acc_t)1 << 21;
            for (int q = 0; q < n; ++q) acc += Tap<SGN>::mul(k[q], (unsigned)s[q]);
            T[r * a.t_pitch + e] = (unsigned char)Tap<SGN>::clip(acc);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();
    mode_height_pass<CO, OutT, SGN, false, PLACED>(a, im, img, T, mode_tile<CO, OutT>(a, smem), lut, Y.lo, Y.cnt, Y.k, Y.ks, ya, ox0, oy0, ncols, oy1 - oy0, tid,
                                                     lx_cnt, fill_arg(fill...));
}

// X-major source.  LDS as k_resize_xmajor's with T in one component.  A colour source: a lane takes 16 PIXELS of a column — 48
// consecutive bytes, three 16-byte loads — per tap, converts them in registers and accumulates their L.  (The last chunk of a
// column reads up to 47 bytes behind the rows the tile needs: the next column's, or the buffer's 64 bytes of slack.)
template <int CS, int CO, typename OutT, bool SGN, typename... Fill>
__global__ __launch_bounds__(256) void k_resize_xmajor_mode(const ResizeArgs a, Fill... fill) {
    constexpr bool PLACED = sizeof...(Fill) == 1;
    static_assert(sizeof...(Fill) <= 1, "placed instances: one fill word");
    typedef typename Tap<SGN>::acc_t acc_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tiles = a.tiles_x * a.tiles_y;
    const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;      // (launch_resize: the grid's tail is idle)
    if (wg >= (int64_t)a.n_images * tiles) return;
    const int img = (int)(wg / tiles), t = (int)(wg - (int64_t)img * tiles);
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const DevResizeImage im = a.images[img];
    const int ox0 = tx * a.tc, ox1 = min(ox0 + a.tc, a.ow), oy0 = ty * a.tr, oy1 = min(oy0 + a.tr, a.oh);
    const AxisTab X(a.tabs + im.xtab, a.ow), Y(a.tabs + im.ytab, a.oh);
    const int ya = Y.lo[oy0], yb = Y.lo[oy1 - 1] + Y.cnt[oy1 - 1];
    const int nrows = yb - ya, ncols = ox1 - ox0, orows = oy1 - oy0;
    if constexpr (PLACED) { if (X.lo[ox1 - 1] + X.cnt[ox1 - 1] == X.lo[ox0] || yb == ya) { fill_tile<CO, OutT, true>(a, im, img, fill_arg(fill...), ox0, oy0, ncols, orows); return; } }
    unsigned char *T = smem;
    int32_t *ly_lo = reinterpret_cast<int32_t *>(smem + a.tab_off), *ly_cnt = ly_lo + a.tr, *ly_k = ly_cnt + a.tr;
    const int tid = threadIdx.x;
    for (int i = tid; i < orows; i += 256) { ly_lo[i] = Y.lo[oy0 + i] - ya; ly_cnt[i] = Y.cnt[oy0 + i]; }
    for (int i = tid; i < orows * Y.ks; i += 256) ly_k[i] = Y.k[(int64_t)oy0 * Y.ks + i];
    const OutT *lut = stage_lut<CO, OutT>(a, smem, tid);
    const unsigned char *src = a.src + im.src_off;
    const int nch = (nrows + 15) >> 4;                 // 16 pixels of a column per lane
    const int64_t col = (int64_t)im.h * CS;
    for (int i = tid; i < ncols * nch; i += 256) {
        const int oxl = i / nch, j = i - oxl * nch;
        const int ox = ox0 + oxl, n = X.cnt[ox];
        const int32_t *k = X.k + (int64_t)ox * X.ks;
        const unsigned char *p = src + ((int64_t)X.lo[ox] * im.h + ya + 16 * j) * CS;
        acc_t acc[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) acc[b] = (acc_t)1 << 21;
        for (int q = 0; q < n; ++q, p += col) {
            const int32_t kq = k[q];
            if constexpr (CS == 3) {
                unsigned w[12];
                __builtin_memcpy(w, p, 48);
#pragma unroll
                for (int b = 0; b < 16; ++b) {
                    const unsigned r = (w[(3 * b) >> 2] >> (8 * ((3 * b) & 3))) & 255u, g = (w[(3 * b + 1) >> 2] >> (8 * ((3 * b + 1) & 3))) & 255u,
                                   bl = (w[(3 * b + 2) >> 2] >> (8 * ((3 * b + 2) & 3))) & 255u;
                    acc[b] += Tap<SGN>::mul(kq, mode_luma(r, g, bl));
                }
            } else {
                u32x4 v;
                __builtin_memcpy(&v, p, 16);
#pragma unroll
                for (int b = 0; b < 16; ++b) acc[b] += Tap<SGN>::mul(kq, (v[b >> 2] >> (8 * (b & 3))) & 255u);
            }
        }
        u32x4 o;
#pragma unroll
        for (int d = 0; d < 4; ++d)
            o[d] = Tap<SGN>::clip(acc[4 * d]) | Tap<SGN>::clip(acc[4 * d + 1]) << 8 | Tap<SGN>::clip(acc[4 * d + 2]) << 16 | Tap<SGN>::clip(acc[4 * d + 3]) << 24;
        *reinterpret_cast<u32x4 *>(T + oxl * a.t_pitch + 16 * j) = o;
    }
    __syncthreads();
    mode_height_pass<CO, OutT, SGN, true, PLACED>(a, im, img, T, mode_tile<CO, OutT>(a, smem), lut, ly_lo, ly_cnt, ly_k, Y.ks, ya, ox0, oy0, ncols, orows, tid,
                                                    X.cnt + ox0, fill_arg(fill...));
}


}  // namespace

hipError_t launch_resize(hipStream_t stream, const ResizeArgs &a, int ncomp, int out_ncomp, int placed, unsigned fill) {
    if (a.n_images <= 0) return hipSuccess;
    // one workgroup per tile, numbered along x then y: a grid dimension times the block's stays far below the runtime's 2^32
    const int64_t total = (int64_t)a.n_images * a.tiles_x * a.tiles_y, gx = std::min<int64_t>(total, kResizeGridX);
    const dim3 grid((unsigned)gx, (unsigned)((total + gx - 1) / gx)), block(256);
    // a plan that converts (mj_plan_request.mode with a size): grey to RGB, or colour to L
    const bool converts = out_ncomp && out_ncomp != ncomp;
    // how the source is read (transposing orientations: the oriented image's rows are the stored columns — the other layout's
    // way of reading; a.orient is set on plans of oriented-style instances only)
    const bool xmajor = ((a.layout & 1) == 0) != (a.orient == 2);
    // The style of a native instance, <MIRROR, ORIENT>: <false, false> for a plan with a size and nothing else (esize 1, no mirror —
    // the instances that were there before the others), <true, false> with mirror flags, <false, true> the oriented style, whose
    // per-image byte holds both store flips.  There are no signed mirror instances (half the count): a signed plan with mirror
    // flags takes the oriented instance, whose byte holds a mirror flag in bit 0 as it holds an orientation's.  Converting and
    // placed instances exist in the oriented style only (all zero bytes for a plain plan).
    const bool oriented = a.orient || (a.sgn && a.mirror);
    auto go = [&](auto *k, auto... f) { hipLaunchKernelGGL(k, grid, block, a.lds_bytes, stream, a, f...); };
    // Every ladder between what a plan fixes at run time and an instance at compile time is written once: element size -> stored
    // type and taps below zero -> SGN at the bottom, source order and component count in `instance`.
    auto instance = [&](auto e, auto s) {
        typedef decltype(e) OutT;
        constexpr bool SGN = decltype(s)::value;
        // (f: nothing, or a placed plan's fill word — the placed instance)
        auto native = [&](auto m, auto o, auto... f) {
            constexpr bool M = decltype(m)::value, O = decltype(o)::value;
            if (xmajor && ncomp == 3) go(k_resize_xmajor<3, OutT, M, O, SGN, decltype(f)...>, f...);
            else if (xmajor) go(k_resize_xmajor<1, OutT, M, O, SGN, decltype(f)...>, f...);
            else if (ncomp == 3) go(k_resize_rowmajor<3, OutT, M, O, SGN, decltype(f)...>, f...);
            else go(k_resize_rowmajor<1, OutT, M, O, SGN, decltype(f)...>, f...);
        };
        auto mode = [&](auto... f) {
            if (xmajor && ncomp == 1) go(k_resize_xmajor_mode<1, 3, OutT, SGN, decltype(f)...>, f...);
            else if (xmajor) go(k_resize_xmajor_mode<3, 1, OutT, SGN, decltype(f)...>, f...);
            else if (ncomp == 1) go(k_resize_rowmajor_mode<1, 3, OutT, SGN, decltype(f)...>, f...);
            else go(k_resize_rowmajor_mode<3, 1, OutT, SGN, decltype(f)...>, f...);
        };
        const std::true_type yes;
        const std::false_type no;
        if (converts) { if (placed) mode(fill); else mode(); }
        else if (placed) native(no, yes, fill);
        else if (oriented) native(no, yes);
        else if (a.mirror) { if constexpr (!SGN) native(yes, no); }
        else native(no, no);
    };
    auto sign = [&](auto e) { if (a.sgn) instance(e, std::true_type{}); else instance(e, std::false_type{}); };
    if (a.esize == 4) sign(uint32_t{});
    else if (a.esize == 2) sign(uint16_t{});
    else sign((unsigned char)0);
    return hipGetLastError();
}

// ---- host: the output table -------------------------------------------------------------------------------------------
namespace {

uint32_t float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// float32 -> float16, round to nearest even (overflow to infinity, gradual underflow)
uint16_t half_bits(float f) {
    const uint32_t x = float_bits(f), sign = (x >> 16) & 0x8000u, m = x & 0x7FFFFFFFu;
    if (m > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);                 // NaN
    if (m >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);                // 65520 and above, infinity
    if (m < 0x38800000u) {
        // below 2^-14: adding 0.5 leaves the value in units of 2^-24 — float16's subnormal step — in the low mantissa
        // bits, rounded to nearest even by the addition itself
        float a;
        memcpy(&a, &m, 4);
        volatile float sum = a + 0.5f;
        return (uint16_t)(sign | (float_bits(sum) - 0x3F000000u));
    }
    const uint32_t r = m - 0x38000000u + 0xFFFu + ((m >> 13) & 1u);         // exponent rebias, then half an ulp (ties to even)
    return (uint16_t)(sign | (r >> 13));
}

uint16_t bfloat_bits(float f) {
    const uint32_t x = float_bits(f);
    if ((x & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((x >> 16) | 0x40u);
    return (uint16_t)((x + 0x7FFFu + ((x >> 16) & 1u)) >> 16);
}

}  // namespace

// Every operation a float32 one, each rounded on its own (this library is built with -ffp-contract=off; the volatiles keep
// a host compiler from carrying more precision between them).
void build_normalize_table(int dtype, float mean, float std, uint32_t *bits) {
    for (int v = 0; v < 256; ++v) {
        volatile float t = (float)v / 255.0f;
        volatile float d = t - mean;
        volatile float y = d / std;
        bits[v] = dtype == MJ_DTYPE_F32 ? float_bits(y) : dtype == MJ_DTYPE_F16 ? half_bits(y) : bfloat_bits(y);
    }
}

}  // namespace mj
