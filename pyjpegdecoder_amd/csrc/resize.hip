// Decode to a fixed size: the batch's decoded pixels (whole images or windows, as stage 2 packed them) resized to one
// out_width x out_height, all images in ONE launch, into one dense output.
//
// The arithmetic is Pillow's Image.resize(size, filter) on 8-bit data (tools/resize_model.py restates it) for BILINEAR — the
// default — BOX, HAMMING, BICUBIC and LANCZOS (mj_plan_create_resized_filtered): per axis a
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
// Model-ready output (mj_plan_create_resized_as): the height pass ends in a byte v of component c, and what it stores is a
// pure function of (c, v) — torchvision's Normalize(mean, std)(to_tensor(img)) in float32, operation by operation, then
// rounded to nearest even for the 16-bit types (tools/normalize_model.py).  The host evaluates it for the 256 x C pairs
// (build_normalize_table) and the kernels' 2- and 4-byte instances store lut[c][v] out of LDS: exact by construction, no
// float arithmetic on the device.  float16 and bfloat16 share the 2-byte instance (the table holds the bits).  Mirror is a
// per-image flag (ResizeArgs::mirror) of the mirror instances: the element goes to column out_width - 1 - x.  A lane still stores one element
// and consecutive lanes consecutive elements of the output's contiguous axis, so a wavefront's store is one run of 64, 128
// or 256 bytes (descending for a mirrored image of a row-major layout); the plain uint8 instances are the code they were.
//
// Output colour mode (mj_plan_create_resized_mode): the k_resize_*_mode instances, whose source has CS components and whose
// output CO — greyscale files into three components (Pillow's convert("RGB")) and colour files into one (convert("L"),
// mode_luma of the decoded RGB bytes).  The conversion comes first, as in img.convert(mode).resize(size): colour to L where the
// source is read, before any tap (the staged row in LDS; 16 pixels = 48 bytes per lane and tap in registers), so both passes and
// T run on ONE component either way.  Grey to RGB finishes every pixel's sum once into a tile of bytes in LDS and the store
// loop — one element per lane, consecutive lanes consecutive elements, as above — looks up lut[c][byte] for c = 0..2.  They
// are instances in the oriented style only (the per-image byte holds the flips and the mirror flag; all zero for a plain plan).
//
// Aspect-preserving sizing (mj_plan_create_resized_placed): the output is a canvas, every image is resized to a size of its own and
// placed at an offset on it; elements it does not cover hold a fill byte, which takes the output's path like any other.  The tap
// tables are built in the canvas's coordinates — an entry outside the image has no taps and keeps the bound of the nearest entry inside
// as its first index — so the k_resize_*_placed instances compute canvas elements only: a tile the image does not reach stores
// fill and returns before any staging, a tile it reaches runs the width pass over the covered columns and rows alone.  With windows,
// plan creation shrinks every window to the source range the canvas needs (create_resized: the rule and its numbers).
#include <math.h>

#include <map>

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

int resize_axis_ksize(int in_size, int out_size, int filter) {
    const double scale = (double)in_size / (double)out_size;
    const double support = kFilters[filter].support * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}

void build_resize_axis(int in_size, int out_size, int32_t *xmin, int32_t *count, int32_t *taps, int taps_stride, int filter) {
    const FilterDef &F = kFilters[filter];
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = F.support * filterscale, ss = 1.0 / filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    std::vector<double> w((size_t)ksize + 2);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
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

// ---- placed plans (mj_plan_create_resized_placed): `fill` holds the canvas's fill byte of component c in bits 8c..8c+7
__device__ __forceinline__ unsigned fill_byte(unsigned fill, int c) { return (fill >> (8 * c)) & 255u; }

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
template <int C, typename OutT = unsigned char, bool MIRROR = false, bool ORIENT = false, bool SGN = false>
__global__ __launch_bounds__(256) void k_resize_rowmajor(const ResizeArgs a) {
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
        if constexpr (ORIENT) dst[out_index(a, C, (turn & 1) ? a.ow - 1 - ox : ox, (turn & 2) ? a.oh - 1 - oy : oy, c)] = out_value<OutT>(lut, c, Tap<SGN>::clip(acc));
        else dst[out_index(a, C, flip ? a.ow - 1 - ox : ox, oy, c)] = out_value<OutT>(lut, c, Tap<SGN>::clip(acc));
    }
}

// The placed instance: k_resize_rowmajor in the oriented style (the per-image byte holds the flips and the mirror flag, all zero
// where there are none) over canvas tables — entries outside the image have no taps and keep the bound of the nearest entry
// inside as their first index, so a tile's span covers only what the image needs and the width pass runs over that alone.
template <int C, typename OutT, bool SGN>
__global__ __launch_bounds__(256) void k_resize_rowmajor_placed(const ResizeArgs a, const unsigned fill) {
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
    if (xb == xa || yb == ya) { fill_tile<C, OutT, false>(a, im, img, fill, ox0, oy0, ncols, oy1 - oy0); return; }
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
    const unsigned turn = a.mirror[img];      // bit 0 = store at column ow - 1 - x, bit 1 = at row oh - 1 - y
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
        // (no taps on either axis: a canvas element the image does not cover)
        const unsigned v = (n == 0 || lx_cnt[oxl] == 0) ? fill_byte(fill, c) : Tap<SGN>::clip(acc);
        dst[out_index(a, C, (turn & 1) ? a.ow - 1 - ox : ox, (turn & 2) ? a.oh - 1 - oy : oy, c)] = out_value<OutT>(lut, c, v);
    }
}

// X-major source.  LDS: T [tc][t_pitch] (one row per output column: the bytes (y, c) of the source rows the tile needs,
// t_pitch a multiple of 16) | per output row of the tile: first source row (relative), taps, the taps themselves [tr][ksy] |
// the output table (2- and 4-byte elements).
template <int C, typename OutT = unsigned char, bool MIRROR = false, bool ORIENT = false, bool SGN = false>
__global__ __launch_bounds__(256) void k_resize_xmajor(const ResizeArgs a) {
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
        if constexpr (ORIENT) dst[out_index(a, C, (turn & 1) ? a.ow - 1 - ox : ox, (turn & 2) ? a.oh - 1 - (oy0 + oyl) : oy0 + oyl, c)] = out_value<OutT>(lut, c, Tap<SGN>::clip(acc));
        else dst[out_index(a, C, flip ? a.ow - 1 - ox : ox, oy0 + oyl, c)] = out_value<OutT>(lut, c, Tap<SGN>::clip(acc));
    }
}

// The placed instance (as k_resize_rowmajor_placed)
template <int C, typename OutT, bool SGN>
__global__ __launch_bounds__(256) void k_resize_xmajor_placed(const ResizeArgs a, const unsigned fill) {
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
    if (X.lo[ox1 - 1] + X.cnt[ox1 - 1] == X.lo[ox0] || yb == ya) { fill_tile<C, OutT, true>(a, im, img, fill, ox0, oy0, ncols, orows); return; }
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
    const unsigned turn = a.mirror[img];      // bit 0 = store at column ow - 1 - x, bit 1 = at row oh - 1 - y
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
        // (no taps on either axis: a canvas element the image does not cover)
        const unsigned v = (n == 0 || X.cnt[ox] == 0) ? fill_byte(fill, c) : Tap<SGN>::clip(acc);
        dst[out_index(a, C, (turn & 1) ? a.ow - 1 - ox : ox, (turn & 2) ? a.oh - 1 - (oy0 + oyl) : oy0 + oyl, c)] = out_value<OutT>(lut, c, v);
    }
}

// ---- output colour mode: source components CS != output components CO (T, both passes and the tile geometry: one component)
// The end of the height pass.  CO == 1: the finished byte is the element.  CO == 3: every pixel's byte goes into the tile O in LDS
// once; after the barrier a lane stores one element (pixel, c), looked up in component c's table.
// XM: T is [column][t_pitch] and a tile is walked along its columns (the x-major kernel), else [row][t_pitch] along its rows.
// PLACED: xcnt[oxl] is the tap count of the tile's column oxl — 0 there, or on the height axis, marks an element the image does
// not cover, stored as the fill byte of its component (`fill`: fill_byte).
template <int CO, typename OutT, bool SGN, bool XM, bool PLACED = false>
__device__ __forceinline__ void mode_height_pass(const ResizeArgs &a, const DevResizeImage &im, int img, const unsigned char *T, unsigned char *O,
                                                 const OutT *lut, const int32_t *lo, const int32_t *cnt, const int32_t *k_all, int ks, int ya, int ox0,
                                                 int oy0, int ncols, int orows, int tid, const int32_t *xcnt = nullptr, unsigned fill = 0) {
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
template <int CS, int CO, typename OutT, bool SGN>
__global__ __launch_bounds__(256) void k_resize_rowmajor_mode(const ResizeArgs a) {
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
    mode_height_pass<CO, OutT, SGN, false>(a, im, img, T, mode_tile<CO, OutT>(a, smem), lut, Y.lo, Y.cnt, Y.k, Y.ks, ya, ox0, oy0, ncols, oy1 - oy0, tid);
}

// The placed instance (as k_resize_rowmajor_placed)
template <int CS, int CO, typename OutT, bool SGN>
__global__ __launch_bounds__(256) void k_resize_rowmajor_mode_placed(const ResizeArgs a, const unsigned fill) {
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
    if (xb == xa || yb == ya) { fill_tile<CO, OutT, false>(a, im, img, fill, ox0, oy0, ncols, oy1 - oy0); return; }
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
    mode_height_pass<CO, OutT, SGN, false, true>(a, im, img, T, mode_tile<CO, OutT>(a, smem), lut, Y.lo, Y.cnt, Y.k, Y.ks, ya, ox0, oy0, ncols, oy1 - oy0, tid,
                                                   lx_cnt, fill);
}

// X-major source.  LDS as k_resize_xmajor's with T in one component.  A colour source: a lane takes 16 PIXELS of a column — 48
// consecutive bytes, three 16-byte loads — per tap, converts them in registers and accumulates their L.  (The last chunk of a
// column reads up to 47 bytes behind the rows the tile needs: the next column's, or the buffer's 64 bytes of slack.)
template <int CS, int CO, typename OutT, bool SGN>
__global__ __launch_bounds__(256) void k_resize_xmajor_mode(const ResizeArgs a) {
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
    mode_height_pass<CO, OutT, SGN, true>(a, im, img, T, mode_tile<CO, OutT>(a, smem), lut, ly_lo, ly_cnt, ly_k, Y.ks, ya, ox0, oy0, ncols, orows, tid);
}

// The placed instance (as k_resize_rowmajor_placed)
template <int CS, int CO, typename OutT, bool SGN>
__global__ __launch_bounds__(256) void k_resize_xmajor_mode_placed(const ResizeArgs a, const unsigned fill) {
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
    if (X.lo[ox1 - 1] + X.cnt[ox1 - 1] == X.lo[ox0] || yb == ya) { fill_tile<CO, OutT, true>(a, im, img, fill, ox0, oy0, ncols, orows); return; }
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
    mode_height_pass<CO, OutT, SGN, true, true>(a, im, img, T, mode_tile<CO, OutT>(a, smem), lut, ly_lo, ly_cnt, ly_k, Y.ks, ya, ox0, oy0, ncols, orows, tid,
                                                  X.cnt + ox0, fill);
}


template <int CS, int CO, typename OutT>
void launch_mode_instance(hipStream_t stream, const ResizeArgs &a, dim3 grid, dim3 block, int placed, unsigned fill) {
    const bool xmajor = ((a.layout & 1) == 0) != (a.orient == 2);      // (as launch_instance: transposing orientations read the other way)
    if (placed) {
        if (xmajor && a.sgn) hipLaunchKernelGGL((k_resize_xmajor_mode_placed<CS, CO, OutT, true>), grid, block, a.lds_bytes, stream, a, fill);
        else if (xmajor) hipLaunchKernelGGL((k_resize_xmajor_mode_placed<CS, CO, OutT, false>), grid, block, a.lds_bytes, stream, a, fill);
        else if (a.sgn) hipLaunchKernelGGL((k_resize_rowmajor_mode_placed<CS, CO, OutT, true>), grid, block, a.lds_bytes, stream, a, fill);
        else hipLaunchKernelGGL((k_resize_rowmajor_mode_placed<CS, CO, OutT, false>), grid, block, a.lds_bytes, stream, a, fill);
        return;
    }
    if (xmajor && a.sgn) hipLaunchKernelGGL((k_resize_xmajor_mode<CS, CO, OutT, true>), grid, block, a.lds_bytes, stream, a);
    else if (xmajor) hipLaunchKernelGGL((k_resize_xmajor_mode<CS, CO, OutT, false>), grid, block, a.lds_bytes, stream, a);
    else if (a.sgn) hipLaunchKernelGGL((k_resize_rowmajor_mode<CS, CO, OutT, true>), grid, block, a.lds_bytes, stream, a);
    else hipLaunchKernelGGL((k_resize_rowmajor_mode<CS, CO, OutT, false>), grid, block, a.lds_bytes, stream, a);
}

// the instance of one output element and mirror mode: source order and component count picked at run time
template <typename OutT, bool MIRROR, bool ORIENT = false, bool SGN = false>
void launch_instance(hipStream_t stream, const ResizeArgs &a, int ncomp, dim3 grid, dim3 block) {
    // (transposing orientations: the oriented image's rows are the stored columns — the other layout's way of reading)
    const bool xmajor = ((a.layout & 1) == 0) != (ORIENT && a.orient == 2);
    if (xmajor && ncomp == 3) hipLaunchKernelGGL((k_resize_xmajor<3, OutT, MIRROR, ORIENT, SGN>), grid, block, a.lds_bytes, stream, a);
    else if (xmajor) hipLaunchKernelGGL((k_resize_xmajor<1, OutT, MIRROR, ORIENT, SGN>), grid, block, a.lds_bytes, stream, a);
    else if (ncomp == 3) hipLaunchKernelGGL((k_resize_rowmajor<3, OutT, MIRROR, ORIENT, SGN>), grid, block, a.lds_bytes, stream, a);
    else hipLaunchKernelGGL((k_resize_rowmajor<1, OutT, MIRROR, ORIENT, SGN>), grid, block, a.lds_bytes, stream, a);
}

// the signed instances of one output element: plain, or — for a mirrored or an oriented plan alike — the oriented instance,
// whose per-image byte holds a mirror flag in bit 0 as it holds an orientation's (no signed mirror instances: half the count)
template <typename OutT>
void launch_signed(hipStream_t stream, const ResizeArgs &a, int ncomp, dim3 grid, dim3 block) {
    if (a.mirror) launch_instance<OutT, false, true, true>(stream, a, ncomp, grid, block);
    else launch_instance<OutT, false, false, true>(stream, a, ncomp, grid, block);
}

// the placed instances of one output element (as launch_instance picks: source order, component count, signed taps)
template <typename OutT, bool SGN>
void launch_placed_sgn(hipStream_t stream, const ResizeArgs &a, int ncomp, dim3 grid, dim3 block, unsigned fill) {
    const bool xmajor = ((a.layout & 1) == 0) != (a.orient == 2);
    if (xmajor && ncomp == 3) hipLaunchKernelGGL((k_resize_xmajor_placed<3, OutT, SGN>), grid, block, a.lds_bytes, stream, a, fill);
    else if (xmajor) hipLaunchKernelGGL((k_resize_xmajor_placed<1, OutT, SGN>), grid, block, a.lds_bytes, stream, a, fill);
    else if (ncomp == 3) hipLaunchKernelGGL((k_resize_rowmajor_placed<3, OutT, SGN>), grid, block, a.lds_bytes, stream, a, fill);
    else hipLaunchKernelGGL((k_resize_rowmajor_placed<1, OutT, SGN>), grid, block, a.lds_bytes, stream, a, fill);
}
template <typename OutT>
void launch_placed(hipStream_t stream, const ResizeArgs &a, int ncomp, dim3 grid, dim3 block, unsigned fill) {
    if (a.sgn) launch_placed_sgn<OutT, true>(stream, a, ncomp, grid, block, fill);
    else launch_placed_sgn<OutT, false>(stream, a, ncomp, grid, block, fill);
}

}  // namespace

hipError_t launch_resize(hipStream_t stream, const ResizeArgs &a, int ncomp, int out_ncomp, int placed, unsigned fill) {
    if (a.n_images <= 0) return hipSuccess;
    // one workgroup per tile, numbered along x then y: a grid dimension times the block's stays far below the runtime's 2^32
    const int64_t total = (int64_t)a.n_images * a.tiles_x * a.tiles_y, gx = std::min<int64_t>(total, kResizeGridX);
    const dim3 grid((unsigned)gx, (unsigned)((total + gx - 1) / gx)), block(256);
    if (out_ncomp && out_ncomp != ncomp) {       // a plan that converts (mj_plan_create_resized_mode): grey to RGB, or colour to L
        if (ncomp == 1) {
            if (a.esize == 4) launch_mode_instance<1, 3, uint32_t>(stream, a, grid, block, placed, fill);
            else if (a.esize == 2) launch_mode_instance<1, 3, uint16_t>(stream, a, grid, block, placed, fill);
            else launch_mode_instance<1, 3, unsigned char>(stream, a, grid, block, placed, fill);
        } else {
            if (a.esize == 4) launch_mode_instance<3, 1, uint32_t>(stream, a, grid, block, placed, fill);
            else if (a.esize == 2) launch_mode_instance<3, 1, uint16_t>(stream, a, grid, block, placed, fill);
            else launch_mode_instance<3, 1, unsigned char>(stream, a, grid, block, placed, fill);
        }
        return hipGetLastError();
    }
    if (placed) {       // placed plans: instances of their own, in the oriented style
        if (a.esize == 4) launch_placed<uint32_t>(stream, a, ncomp, grid, block, fill);
        else if (a.esize == 2) launch_placed<uint16_t>(stream, a, ncomp, grid, block, fill);
        else launch_placed<unsigned char>(stream, a, ncomp, grid, block, fill);
        return hipGetLastError();
    }
    if (a.sgn) {        // bicubic and Lanczos plans: the signed instances
        if (a.esize == 4) launch_signed<uint32_t>(stream, a, ncomp, grid, block);
        else if (a.esize == 2) launch_signed<uint16_t>(stream, a, ncomp, grid, block);
        else launch_signed<unsigned char>(stream, a, ncomp, grid, block);
        return hipGetLastError();
    }
    if (a.orient) {     // oriented plans: instances of their own (the per-image byte holds both store flips)
        if (a.esize == 4) launch_instance<uint32_t, false, true>(stream, a, ncomp, grid, block);
        else if (a.esize == 2) launch_instance<uint16_t, false, true>(stream, a, ncomp, grid, block);
        else launch_instance<unsigned char, false, true>(stream, a, ncomp, grid, block);
        return hipGetLastError();
    }
    // (a plan of mj_plan_create_resized: esize 1, no mirror — the instances that were there before the others)
    if (a.esize == 4) { if (a.mirror) launch_instance<uint32_t, true>(stream, a, ncomp, grid, block); else launch_instance<uint32_t, false>(stream, a, ncomp, grid, block); }
    else if (a.esize == 2) { if (a.mirror) launch_instance<uint16_t, true>(stream, a, ncomp, grid, block); else launch_instance<uint16_t, false>(stream, a, ncomp, grid, block); }
    else if (a.mirror) launch_instance<unsigned char, true>(stream, a, ncomp, grid, block);
    else launch_instance<unsigned char, false>(stream, a, ncomp, grid, block);
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

// ---- host: mj_plan_create_resized ---------------------------------------------------------------------------------------
namespace {

struct AxisHost {
    std::vector<int32_t> lo, cnt;
    int ks = 0, word_off = 0, in_size = 0;
    // the most source entries a tile of `tile` outputs needs
    int span(int tile) const {
        int m = 0;
        const int out = (int)lo.size();
        for (int o0 = 0; o0 < out; o0 += tile) {
            int hi = 0;
            for (int o = o0; o < std::min(o0 + tile, out); ++o) hi = std::max(hi, lo[o] + cnt[o]);
            m = std::max(m, hi - lo[o0]);
        }
        return m;
    }
};

int round16(int64_t v) { return (int)((v + 15) & ~(int64_t)15); }

int dtype_size(int dtype) { return dtype == MJ_DTYPE_U8 ? 1 : dtype == MJ_DTYPE_F32 ? 4 : 2; }

// what mj_plan_create_resized_as and mj_host_normalize_table refuse: nullptr when `o` is fine, else the reason
const char *output_fault(int dtype, bool normalize, int ncomp, const float *mean, const float *std) {
    if (dtype != MJ_DTYPE_U8 && dtype != MJ_DTYPE_F16 && dtype != MJ_DTYPE_BF16 && dtype != MJ_DTYPE_F32) return "dtype is none of MJ_DTYPE_U8 / F16 / BF16 / F32";
    if (!normalize) return nullptr;
    if (dtype == MJ_DTYPE_U8) return "normalize needs a float dtype (MJ_DTYPE_U8 stores the resized bytes)";
    for (int c = 0; c < ncomp; ++c) {
        if (!std::isfinite(mean[c])) return "mean must be finite";
        if (!std::isfinite(std[c]) || !(std[c] > 0.0f)) return "std must be finite and > 0";
    }
    return nullptr;
}

int create_resized(const char *fn, mj_context *ctx, const mj_batch *b, const mj_roi *rois, int32_t out_width, int32_t out_height,
                   const int32_t *slots, int32_t n_slots, const mj_output_desc *output, const uint8_t *orient, int filter, mj_plan **out, int mode = 0,
                   const mj_place *places = nullptr, const uint8_t *fill = nullptr);

// ... of the oriented images: the orientations checked (NULL, or all of them 1: a plan without them)
int create_resized_oriented(const char *fn, mj_context *ctx, const mj_batch *b, const mj_roi *rois, int32_t out_width, int32_t out_height,
                            const int32_t *slots, int32_t n_slots, const mj_output_desc *output, const uint8_t *orientations, int filter,
                            mj_plan **out, int mode = 0, const mj_place *places = nullptr, const uint8_t *fill = nullptr) {
    bool upright = true;
    for (int i = 0; orientations && b && i < b->n_images; ++i) {
        if (orientations[i] < 1 || orientations[i] > 8)
            return fail(ctx, MJ_ERR_INVALID, "%s: image %d: orientation %d (must be 1..8)", fn, i, (int)orientations[i]);
        upright = upright && orientations[i] == 1;
    }
    return create_resized(fn, ctx, b, rois, out_width, out_height, slots, n_slots, output, upright ? nullptr : orientations, filter, out, mode, places, fill);
}

}  // namespace

extern "C" {

int mj_host_resize_table_filtered(int32_t filter, int32_t in_size, int32_t out_size, int32_t *xmin, int32_t *count, int32_t *taps,
                                  int32_t taps_stride, int32_t *ksize_out) {
    if (!mj::resize_filter_known(filter) || in_size < 1 || out_size < 1 || in_size > 65535 || out_size > 65535) return MJ_ERR_INVALID;
    const int ks = mj::resize_axis_ksize(in_size, out_size, filter);
    if (ksize_out) *ksize_out = ks;
    if (!xmin && !count && !taps) return MJ_OK;
    if (!xmin || !count || !taps || taps_stride < ks) return MJ_ERR_INVALID;
    mj::build_resize_axis(in_size, out_size, xmin, count, taps, taps_stride, filter);
    return MJ_OK;
}

int mj_host_resize_table(int32_t in_size, int32_t out_size, int32_t *xmin, int32_t *count, int32_t *taps, int32_t taps_stride,
                         int32_t *ksize_out) {
    return mj_host_resize_table_filtered(MJ_FILTER_BILINEAR, in_size, out_size, xmin, count, taps, taps_stride, ksize_out);
}

int mj_host_normalize_table(int32_t dtype, float mean, float std, void *out) {
    if (!out || dtype == MJ_DTYPE_U8 || output_fault(dtype, true, 1, &mean, &std)) return MJ_ERR_INVALID;
    uint32_t bits[256];
    mj::build_normalize_table(dtype, mean, std, bits);
    for (int v = 0; v < 256; ++v) {
        if (dtype == MJ_DTYPE_F32) static_cast<uint32_t *>(out)[v] = bits[v];
        else static_cast<uint16_t *>(out)[v] = (uint16_t)bits[v];
    }
    return MJ_OK;
}

int mj_plan_create_resized(mj_context *ctx, const mj_batch *b, const mj_roi *rois, int32_t out_width, int32_t out_height,
                           const int32_t *slots, int32_t n_slots, mj_plan **out) {
    return create_resized("mj_plan_create_resized", ctx, b, rois, out_width, out_height, slots, n_slots, nullptr, nullptr, MJ_FILTER_BILINEAR, out);
}

int mj_plan_create_resized_as(mj_context *ctx, const mj_batch *b, const mj_roi *rois, int32_t out_width, int32_t out_height,
                              const int32_t *slots, int32_t n_slots, const mj_output_desc *output, mj_plan **out) {
    return create_resized("mj_plan_create_resized_as", ctx, b, rois, out_width, out_height, slots, n_slots, output, nullptr, MJ_FILTER_BILINEAR, out);
}

int mj_plan_create_resized_oriented(mj_context *ctx, const mj_batch *b, const mj_roi *rois, int32_t out_width, int32_t out_height,
                                    const int32_t *slots, int32_t n_slots, const mj_output_desc *output, const uint8_t *orientations,
                                    mj_plan **out) {
    return create_resized_oriented("mj_plan_create_resized_oriented", ctx, b, rois, out_width, out_height, slots, n_slots, output, orientations,
                                   MJ_FILTER_BILINEAR, out);
}

int mj_plan_create_resized_filtered(mj_context *ctx, const mj_batch *b, const mj_roi *rois, int32_t out_width, int32_t out_height,
                                    const int32_t *slots, int32_t n_slots, const mj_output_desc *output, const uint8_t *orientations,
                                    int32_t filter, mj_plan **out) {
    const char *fn = "mj_plan_create_resized_filtered";
    if (!mj::resize_filter_known(filter)) return fail(ctx, MJ_ERR_INVALID, "%s: filter %d is none of MJ_FILTER_*", fn, filter);
    return create_resized_oriented(fn, ctx, b, rois, out_width, out_height, slots, n_slots, output, orientations, filter, out);
}

int mj_plan_create_resized_mode(mj_context *ctx, const mj_batch *b, const mj_roi *rois, int32_t out_width, int32_t out_height,
                                const int32_t *slots, int32_t n_slots, const mj_output_desc *output, const uint8_t *orientations,
                                int32_t filter, int32_t mode, mj_plan **out) {
    const char *fn = "mj_plan_create_resized_mode";
    if (!mj::resize_filter_known(filter)) return fail(ctx, MJ_ERR_INVALID, "%s: filter %d is none of MJ_FILTER_*", fn, filter);
    if (mode != MJ_MODE_NATIVE && mode != MJ_MODE_L && mode != MJ_MODE_RGB) return fail(ctx, MJ_ERR_INVALID, "%s: mode %d is none of MJ_MODE_*", fn, mode);
    // (the files' own count: the plan of mj_plan_create_resized_filtered, made by the code that makes it there)
    if (mode == mj::batch_ncomp(b)) mode = MJ_MODE_NATIVE;
    return create_resized_oriented(fn, ctx, b, rois, out_width, out_height, slots, n_slots, output, orientations, filter, out, mode);
}

int mj_plan_create_resized_placed(mj_context *ctx, const mj_batch *b, const mj_roi *rois, int32_t out_width, int32_t out_height,
                                  const int32_t *slots, int32_t n_slots, const mj_output_desc *output, const uint8_t *orientations,
                                  int32_t filter, int32_t mode, const mj_place *places, const uint8_t fill[3], mj_plan **out) {
    const char *fn = "mj_plan_create_resized_placed";
    if (!mj::resize_filter_known(filter)) return fail(ctx, MJ_ERR_INVALID, "%s: filter %d is none of MJ_FILTER_*", fn, filter);
    if (mode != MJ_MODE_NATIVE && mode != MJ_MODE_L && mode != MJ_MODE_RGB) return fail(ctx, MJ_ERR_INVALID, "%s: mode %d is none of MJ_MODE_*", fn, mode);
    if (mode == mj::batch_ncomp(b)) mode = MJ_MODE_NATIVE;
    // (every image stretched over the whole canvas: the plan of mj_plan_create_resized_mode, made by the code that makes it there)
    bool plain = true;
    for (int i = 0; places && b && i < b->n_images && plain; ++i)
        plain = places[i].width == out_width && places[i].height == out_height && places[i].x == 0 && places[i].y == 0;
    return create_resized_oriented(fn, ctx, b, rois, out_width, out_height, slots, n_slots, output, orientations, filter, out, mode,
                                   plain ? nullptr : places, fill);
}

int mj_debug_resize_shape(const mj_plan *p, int32_t out[8]) {
    if (!p || !out || !p->resized || p->orient_only) return MJ_ERR_INVALID;
    const mj::ResizeArgs &a = p->rz;
    const int32_t v[8] = {a.tr, a.tc, a.tiles_x, a.tiles_y, a.lds_bytes, p->rz_filter, a.sgn, p->rz_max_ksize};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return MJ_OK;
}

}  // extern "C"

namespace {

int create_resized(const char *fn, mj_context *ctx, const mj_batch *b, const mj_roi *rois, int32_t out_width, int32_t out_height,
                   const int32_t *slots, int32_t n_slots, const mj_output_desc *output, const uint8_t *orient, int filter, mj_plan **out, int mode,
                   const mj_place *places, const uint8_t *fill) {
    // (filter: a known MJ_FILTER_*; orient: NULL, or one checked orientation 1..8 per image, not all of them 1; mode: 0, or the
    // output's component count where it is not the batch's; places: NULL, or one per image, not all of them the whole canvas)
    // the output description first: it needs nothing else, not even a context (the message is then mj_last_error(NULL)'s).
    // (A batch's component count is its first image's; all three entries are looked at when there is no image to ask.)
    const int dtype = output ? output->dtype : MJ_DTYPE_U8;
    const int nc_check = mode ? mode : mj::batch_ncomp(b);
    if (output)
        if (const char *why = output_fault(dtype, output->normalize != 0, nc_check, output->mean, output->std))
            return fail(ctx, MJ_ERR_INVALID, "%s: output: %s", fn, why);
    if (!ctx) return MJ_ERR_INVALID;
    if (!b || !out) return fail(ctx, MJ_ERR_INVALID, "%s: NULL argument", fn);
    *out = nullptr;
    const int esize = dtype_size(dtype);
    if (out_width < 1 || out_height < 1 || out_width > 65535 || out_height > 65535)
        return fail(ctx, MJ_ERR_INVALID, "%s: output size %d x %d (both must be 1..65535)", fn, out_width, out_height);
    if (b->flags & (MJ_FLAG_KEEP_PLANES | MJ_FLAG_KEEP_IDCT))
        return fail(ctx, MJ_ERR_INVALID, "%s: the seam outputs (MJ_FLAG_KEEP_PLANES / MJ_FLAG_KEEP_IDCT) are at the files' own sizes; a resized plan has none", fn);
    if (!slots) n_slots = b->n_images;
    for (int i = 0; slots && i < b->n_images; ++i)
        if (slots[i] < 0 || slots[i] >= n_slots)
            return fail(ctx, MJ_ERR_INVALID, "%s: image %d: slot %d outside the %d slots of the output", fn, i, slots[i], n_slots);
    // oriented plans: all images transposing (orientations 5..8) or none — the two read their source in different ways, so
    // they are two launches, i.e. two plans (BatchDecoder sorts the files); windows are given in oriented coordinates
    // Placed plans: what every axis of every image needs of its source — the taps of the canvas entries the image covers reach
    // source entries [first, first + len) of the oriented image or window (need).  Where that is less than the whole, the plan
    // becomes a window plan of that range (derived), as if the caller had asked for it: restart segments and MCUs outside are
    // skipped as mj_plan_create_roi skips them, and the tables are rebased to the range.
    struct Need { int x0, nx, y0, ny, sw, sh; };      // (sw, sh: the oriented image or window the tables are made for)
    std::vector<Need> need;
    std::vector<mj_roi> derived;
    if (places) {
        if (!b->images && b->n_images > 0) return fail(ctx, MJ_ERR_INVALID, "%s: NULL argument", fn);
        need.resize((size_t)b->n_images);
        int64_t area_need = 0, area_all = 0;
        std::map<std::vector<int>, std::pair<int, int>> spans;      // (a batch of one size and one placement: one table per axis)
        for (int i = 0; i < b->n_images; ++i) {
            const mj_place &pl = places[i];
            if (pl.width < 1 || pl.height < 1 || pl.width > 65535 || pl.height > 65535 || pl.x < -65535 || pl.x > 65535 || pl.y < -65535 || pl.y > 65535)
                return fail(ctx, MJ_ERR_INVALID, "%s: image %d: place (width=%d, height=%d, x=%d, y=%d): the size must be 1..65535, the offsets within +-65535",
                            fn, i, pl.width, pl.height, pl.x, pl.y);
            if (pl.x >= out_width || pl.y >= out_height || (int64_t)pl.x + pl.width <= 0 || (int64_t)pl.y + pl.height <= 0)
                return fail(ctx, MJ_ERR_INVALID, "%s: image %d: a %d x %d image at (%d, %d) does not meet the %d x %d canvas", fn, i, pl.width, pl.height,
                            pl.x, pl.y, out_width, out_height);
            const int bits = orient ? mj::orient_bits(orient[i]) : 0;
            int W = b->images[i].width, H = b->images[i].height;
            if (bits & 4) std::swap(W, H);
            mj_roi r = rois ? rois[i] : mj_roi{0, 0, W, H}, tmp;
            need[(size_t)i] = Need{0, r.width, 0, r.height, r.width, r.height};
            // (a window the plan will refuse, or a size no table is built for: left as it is, for the code that refuses it)
            if (W < 1 || H < 1 || W > 65535 || H > 65535 || !mj::stored_window(1, W, H, r, &tmp)) { area_all += 1; area_need += 1; continue; }
            auto span = [&](int in_size, int resized, int off, int canvas, int *first, int *len) {
                const std::vector<int> key{in_size, resized, off, canvas};
                auto it = spans.find(key);
                if (it != spans.end()) { *first = it->second.first; *len = it->second.second; return; }
                std::vector<int32_t> lo((size_t)resized), cnt((size_t)resized);
                const int ks = mj::resize_axis_ksize(in_size, resized, filter);
                std::vector<int32_t> k((size_t)resized * ks);
                mj::build_resize_axis(in_size, resized, lo.data(), cnt.data(), k.data(), ks, filter);
                const int j0 = std::max(0, -off), j1 = std::min(resized, canvas - off) - 1;     // the resized entries on the canvas
                *first = lo[(size_t)j0]; *len = lo[(size_t)j1] + cnt[(size_t)j1] - lo[(size_t)j0];
                spans[key] = {*first, *len};
            };
            Need &nd = need[(size_t)i];
            span(r.width, pl.width, pl.x, out_width, &nd.x0, &nd.nx);
            span(r.height, pl.height, pl.y, out_height, &nd.y0, &nd.ny);
            area_all += (int64_t)r.width * r.height; area_need += (int64_t)nd.nx * nd.ny;
        }
        // The rule: a caller's windows make a window plan anyway, and it shrinks to what is needed.  Whole images stay whole: a
        // window plan does not take the fused launch, and for the evaluation transform of 1024 x 1080p — 44 % of the pixels
        // needed — decoding the window took 11.1 ms (row-major) / 8.9 ms (x-major) against 6.4 / 6.2 ms for the whole images,
        // while the placed launch itself cost the same over either (profiles/r13_place_probe.txt).  MJ_PLACE_WINDOW: 0 never,
        // 1 whenever anything is saved (tests, probes, and crops far smaller than the one measured).
        bool derive = rois != nullptr;
        if (const char *e = mj::opt("MJ_PLACE_WINDOW")) derive = atoi(e) != 0;
        if (derive && area_need < area_all) {
            derived.resize((size_t)b->n_images);
            for (int i = 0; i < b->n_images; ++i) {
                const int bits = orient ? mj::orient_bits(orient[i]) : 0;
                const mj_roi r = rois ? rois[i] : mj_roi{0, 0, (bits & 4) ? b->images[i].height : b->images[i].width,
                                                         (bits & 4) ? b->images[i].width : b->images[i].height};
                const Need &nd = need[(size_t)i];
                derived[(size_t)i] = mj_roi{r.x + nd.x0, r.y + nd.y0, nd.nx, nd.ny};
            }
            rois = derived.data();
        } else {
            for (Need &nd : need) nd.x0 = nd.y0 = 0;       // (tables over the whole image or window)
        }
    }
    bool swapped = false;
    std::vector<mj_roi> stored;
    if (orient) {
        if (!b->images) return fail(ctx, MJ_ERR_INVALID, "%s: NULL argument", fn);
        swapped = b->n_images > 0 && (mj::orient_bits(orient[0]) & 4);
        for (int i = 0; i < b->n_images; ++i)
            if (((mj::orient_bits(orient[i]) & 4) != 0) != swapped)
                return fail(ctx, MJ_ERR_UNSUPPORTED, "%s: image %d: orientations that exchange width and height (5..8) and others do not share a resized plan; split the batch", fn, i);
        if (rois) {
            stored.resize((size_t)b->n_images);
            for (int i = 0; i < b->n_images; ++i)
                if (!mj::stored_window(orient[i], b->images[i].width, b->images[i].height, rois[i], &stored[(size_t)i]))
                    return fail(ctx, MJ_ERR_INVALID, "%s: image %d: window (x=%d, y=%d, width=%d, height=%d) is empty or not inside the oriented image", fn,
                                i, rois[i].x, rois[i].y, rois[i].width, rois[i].height);
            rois = stored.data();
        }
    }
    mj_plan *p = nullptr;
    // (whole images: a plain plan, which may take the fused launch; windows: a window plan)
    if (int rc = mj::plan_create_common(ctx, b, rois, rois != nullptr, &p)) return rc;
    struct Guard { mj_plan *p; ~Guard() { if (p) mj_plan_destroy(p); } } guard{p};
    // C: the source's components.  A plan that converts stores CO of them per pixel and runs both passes, and T, on CT = 1:
    // colour becomes L where it is read, grey becomes RGB where it is stored (resize.hip's k_resize_*_mode)
    const int C = p->ncomp, n = p->n_images, CO = mode ? mode : C, CT = mode ? 1 : C;
    if (mode) p->out_ncomp = CO;
    const int64_t out_image = (int64_t)out_width * out_height * CO * esize;      // bytes
    // tap tables: one per distinct source size and axis
    std::map<int, AxisHost> xs, ys;
    std::vector<int32_t> words;
    // What the kernels' arithmetic holds (resize.hip: Tap): a 24-bit multiply and a 32-bit sum — signed for the filters with side
    // lobes.  Measured over sizes 1..129 the taps stay far inside (tests/test_resample_host.py); that is no proof for every
    // size, so every table is checked and one that breaks a bound is refused (range_in / range_out: its sizes).
    const bool sgn = mj::resize_filter_signed(filter);
    int range_in = 0, range_out = 0;
    // (back: the table of an axis the orientation reverses — entry j is entry out_size - 1 - j of the plain table read from the
    // other end of the source, taps in reverse; the sums are integer sums of the same products, and the first source index
    // still grows with j, which is what the kernels' tile bounds assume.  The kernel stores entry j at out_size - 1 - j.)
    // (placed plans: canvas entry j is entry j - off of the table in_size -> resized, whose first source indices are then
    // counted from `base`, the first entry of the part of the source that was decoded (`len` entries).  A canvas entry outside
    // the image has NO taps, and as first index the bound of the nearest entry inside: the bounds still grow with j, so the
    // kernels' tile spans hold, and a count of 0 on either axis marks a fill element — an entry inside has at least one tap.
    // The canvas table is built first and reversed after.  Tables are then per (source size, resized size, offset, reversed).)
    std::map<std::vector<int>, int> placed_ids;
    auto axis = [&](std::map<int, AxisHost> &m, int in_size, int out_size, bool back = false, int resized = 0, int off = 0, int base = 0,
                    int len = 0) -> const AxisHost & {
        int key = 2 * in_size + (back ? 1 : 0);
        if (places) {
            const std::vector<int> full{&m == &xs, in_size, resized, off, back, base, len};
            auto id = placed_ids.find(full);
            if (id == placed_ids.end()) id = placed_ids.emplace(full, (int)placed_ids.size()).first;
            key = id->second;
        }
        auto it = m.find(key);
        if (it != m.end()) return it->second;
        AxisHost &A = m[key];
        A.in_size = in_size;
        A.lo.resize(out_size); A.cnt.resize(out_size);
        std::vector<int32_t> k;
        if (places) {
            A.ks = mj::resize_axis_ksize(in_size, resized, filter);
            std::vector<int32_t> lo((size_t)resized), cnt((size_t)resized), kk((size_t)resized * A.ks);
            mj::build_resize_axis(in_size, resized, lo.data(), cnt.data(), kk.data(), A.ks, filter);
            k.assign((size_t)out_size * A.ks, 0);
            const int j0 = std::max(0, off), j1 = std::min(out_size, off + resized);       // the canvas entries inside the image
            for (int j = 0; j < out_size; ++j) {
                if (j < j0) { A.lo[j] = lo[(size_t)(j0 - off)] - base; A.cnt[j] = 0; }
                else if (j >= j1) { A.lo[j] = lo[(size_t)(j1 - 1 - off)] + cnt[(size_t)(j1 - 1 - off)] - base; A.cnt[j] = 0; }
                else {
                    A.lo[j] = lo[(size_t)(j - off)] - base; A.cnt[j] = cnt[(size_t)(j - off)];
                    memcpy(&k[(size_t)j * A.ks], &kk[(size_t)(j - off) * A.ks], (size_t)A.ks * sizeof(int32_t));
                }
            }
            in_size = len;      // (what the reversal below counts from: the decoded part's other end)
        } else {
            A.ks = mj::resize_axis_ksize(in_size, out_size, filter);
            k.resize((size_t)out_size * A.ks);
            mj::build_resize_axis(in_size, out_size, A.lo.data(), A.cnt.data(), k.data(), A.ks, filter);
        }
        for (int j = 0; j < out_size && !range_in; ++j) {
            int64_t sum = 0, big = 0, least = 0;
            for (int t = 0; t < A.ks; ++t) {
                const int64_t v = k[(size_t)j * A.ks + t], m = v < 0 ? -v : v;
                sum += m; big = std::max(big, m); least = std::min(least, v);
            }
            const int64_t top = ((int64_t)1 << 21) + 255 * sum;
            if (sgn ? (big >= (1 << 23) || top > INT32_MAX) : (least < 0 || big >= (1 << 24) || top > (int64_t)UINT32_MAX)) { range_in = A.in_size; range_out = places ? resized : out_size; }
        }
        if (back) {
            std::vector<int32_t> lo(A.lo), cnt(A.cnt), kk(k);
            for (int j = 0; j < out_size; ++j) {
                const int s = out_size - 1 - j;
                A.lo[j] = in_size - lo[s] - cnt[s]; A.cnt[j] = cnt[s];
                for (int t = 0; t < A.ks; ++t) k[(size_t)j * A.ks + t] = t < cnt[s] ? kk[(size_t)s * A.ks + cnt[s] - 1 - t] : 0;
            }
        }
        A.word_off = (int)words.size();
        words.push_back(A.ks);
        words.insert(words.end(), A.lo.begin(), A.lo.end());
        words.insert(words.end(), A.cnt.begin(), A.cnt.end());
        words.insert(words.end(), k.begin(), k.end());
        return A;
    };
    std::vector<mj::DevResizeImage> ri((size_t)n);
    std::vector<uint8_t> flags((size_t)n, 0);      // mirror, per image
    int any_mirror = 0;
    for (int i = 0; i < n; ++i) {
        int w = p->windowed ? p->h_win[i].w : p->h_images[i].width, h = p->windowed ? p->h_win[i].h : p->h_images[i].height;
        const int bits = orient ? mj::orient_bits(orient[i]) : 0;
        if (bits & 4) std::swap(w, h);      // (from here on the oriented image's size)
        ri[i].src_off = p->h_images[i].rgb_off;
        ri[i].dst_off = (int64_t)(slots ? slots[i] : i) * out_image;
        if (mode) p->h_out_off.push_back(ri[i].dst_off);
        ri[i].w = w; ri[i].h = h;
        if (output && output->mirror) any_mirror |= (flags[i] = output->mirror[i] ? 1 : 0);
        if (orient) flags[i] = (uint8_t)((flags[i] ^ (bits & 1)) | (bits & 2));      // (the mirror comes after the orientation)
        if (places) {
            // (w, h: what was decoded of the oriented image — the whole, the caller's window, or the derived range of either)
            const Need &nd = need[(size_t)i];
            ri[i].xtab = axis(xs, nd.sw, out_width, bits & 1, places[i].width, places[i].x, nd.x0, w).word_off;
            ri[i].ytab = axis(ys, nd.sh, out_height, bits & 2, places[i].height, places[i].y, nd.y0, h).word_off;
        } else {
            ri[i].xtab = axis(xs, w, out_width, bits & 1).word_off;
            ri[i].ytab = axis(ys, h, out_height, bits & 2).word_off;
        }
        if (range_in)
            return fail(ctx, MJ_ERR_UNSUPPORTED, "%s: resizing %d to %d with filter %d gives taps outside what the kernels' 24-bit products and 32-bit sums hold", fn,
                        range_in, range_out, filter);
        if (words.size() > ((size_t)1 << 28)) return fail(ctx, MJ_ERR_UNSUPPORTED, "%s: the tap tables of this batch are too large", fn);
    }
    // (a pure function of the tile: what it takes in LDS and where the parts lie; nothing is kept until a tile is chosen)
    struct Lds { bool ok; int t_pitch, tab_off, stage_off, stage_bytes, lut_off, total; };
    const int lut_bytes = esize > 1 ? 256 * CO * esize : 0;
    // The tile: what a workgroup's LDS holds (resize.hip's kernels) must fit 64 KB — the intermediate rows of the tile, the
    // tile's tap tables, the staging rows, the output table of a 2- or 4-byte element — for every source size of the batch.  Tiles shrink until it does: a row-major plan
    // gives up columns first while a row segment stays 2 KB long (its loads run along the rows), then rows; an x-major plan
    // keeps its rows (its loads run along the columns) and gives up columns.
    // (how the source is read, which for transposing orientations is the other layout's way: launch_instance)
    const bool xmajor = ((p->layout & 1) == 0) != swapped;
    mj::ResizeArgs &a = p->rz;
    a = mj::ResizeArgs{};
    int tr = std::min<int>(xmajor ? 32 : 16, out_height), tc = out_width;
    const int budget = 64 * 1024;
    auto lds_for = [&](int tr_, int tc_) -> Lds {
        int sy = 0, sx = 0, ksx = 0, ksy = 0, pitch;
        for (auto &kv : ys) { sy = std::max(sy, kv.second.span(tr_)); ksy = std::max(ksy, kv.second.ks); }
        for (auto &kv : xs) { sx = std::max(sx, kv.second.span(tc_)); ksx = std::max(ksx, kv.second.ks); }
        int64_t t_bytes, tab_bytes, stage = 0;
        if (xmajor) {
            pitch = round16((int64_t)sy * CT);
            t_bytes = (int64_t)tc_ * pitch;
            tab_bytes = ((int64_t)2 * tr_ + (int64_t)tr_ * ksy) * 4;
        } else {
            pitch = round16((int64_t)tc_ * CT);
            t_bytes = (int64_t)sy * pitch;
            tab_bytes = ((int64_t)2 * tc_ + (int64_t)tc_ * ksx) * 4;
            // (colour to L: three quarters for the staged colour row — 3 * (sx + 16) >= 3 * sx + 32 —, one for its L bytes)
            stage = mode && C == 3 ? 4 * (int64_t)round16((int64_t)sx + 16) : round16((int64_t)sx * C + 32);
        }
        // (grey to RGB: the tile of finished bytes behind the output table)
        const int64_t lut_off = t_bytes + round16(tab_bytes) + 4 * stage, total = lut_off + lut_bytes + (mode && C == 1 ? (int64_t)tr_ * tc_ : 0);
        if (total > budget) return Lds{false, 0, 0, 0, 0, 0, 0};
        return Lds{true, pitch, (int)t_bytes, (int)(t_bytes + round16(tab_bytes)), (int)stage, (int)lut_off, (int)total};
    };
    auto fits = [&](int tr_, int tc_) { return lds_for(tr_, tc_).ok; };
    auto seg_bytes = [&](int tc_) { int sx = 0; for (auto &kv : xs) sx = std::max(sx, kv.second.span(tc_)); return sx * C; };
    while (!fits(tr, tc)) {
        const bool cols_first = xmajor ? (tc >= 32 || tr == 1) : (seg_bytes(tc) >= 2048 || tr == 1);
        if (tc > 1 && cols_first) tc = (tc + 1) / 2;
        else if (tr > 1) tr = (tr + 1) / 2;
        else {
            int big_w = 0, big_h = 0;
            for (auto &kv : xs) big_w = std::max(big_w, kv.second.in_size);
            for (auto &kv : ys) big_h = std::max(big_h, kv.second.in_size);
            return fail(ctx, MJ_ERR_UNSUPPORTED, "%s: shrinking %d x %d sources to %d x %d takes more taps per pixel than a workgroup's LDS holds", fn,
                        big_w, big_h, out_width, out_height);
        }
    }
    // (a small batch: more, smaller tiles, so that the chip has something to do)
    auto n_tiles = [&](int tr_, int tc_) { return (int64_t)n * ((out_height + tr_ - 1) / tr_) * ((out_width + tc_ - 1) / tc_); };
    while (n_tiles(tr, tc) < 1024 && tr > 4 && fits((tr + 1) / 2, tc)) tr = (tr + 1) / 2;
    const Lds lds = lds_for(tr, tc);
    a.tr = tr; a.tc = tc;
    a.t_pitch = lds.t_pitch; a.tab_off = lds.tab_off; a.stage_off = lds.stage_off; a.stage_bytes = lds.stage_bytes; a.lds_bytes = lds.total;
    a.esize = esize; a.lut_off = lds.lut_off;
    a.tiles_x = (out_width + tc - 1) / tc; a.tiles_y = (out_height + tr - 1) / tr;
    if (n_tiles(tr, tc) > mj::kResizeGridX * (int64_t)65535)
        return fail(ctx, MJ_ERR_UNSUPPORTED, "%s: %lld tiles are more than one launch takes; split the batch", fn, (long long)n_tiles(tr, tc));
    a.n_images = n; a.ow = out_width; a.oh = out_height; a.layout = p->layout;
    int rc;
    if ((rc = upload(ctx, &p->d_rz_images, ri.data(), ri.size())) != MJ_OK) return rc;
    if ((rc = upload(ctx, &p->d_rz_tabs, words.data(), words.size())) != MJ_OK) return rc;
    a.orient = orient ? (swapped ? 2 : 1) : 0;
    a.sgn = sgn ? 1 : 0;
    p->rz_filter = filter;
    for (auto &kv : xs) p->rz_max_ksize = std::max(p->rz_max_ksize, kv.second.ks);
    for (auto &kv : ys) p->rz_max_ksize = std::max(p->rz_max_ksize, kv.second.ks);
    if (places) {
        p->rz_placed = 1;
        const int nfill = CO;       // (one byte per output component; fill NULL: zeros)
        for (int c = 0; c < nfill && fill; ++c) p->rz_fill |= (unsigned)fill[c] << (8 * c);
    }
    if (any_mirror || orient || mode || places) {       // (no flag set: the instances without mirror; a plan that converts: oriented-style instances only)
        if ((rc = upload(ctx, &p->d_rz_mirror, flags.data(), flags.size())) != MJ_OK) return rc;
        a.mirror = p->d_rz_mirror;
    }
    if (esize > 1) {
        // the output table, [C][256] elements: the host's arithmetic, which the kernels only look up
        const bool norm = output->normalize != 0;
        std::vector<uint8_t> lut((size_t)lut_bytes);
        for (int c = 0; c < CO; ++c) {
            uint32_t bits[256];
            mj::build_normalize_table(dtype, norm ? output->mean[c] : 0.0f, norm ? output->std[c] : 1.0f, bits);
            for (int v = 0; v < 256; ++v) {
                if (esize == 4) memcpy(&lut[((size_t)c * 256 + v) * 4], &bits[v], 4);
                else { const uint16_t h = (uint16_t)bits[v]; memcpy(&lut[((size_t)c * 256 + v) * 2], &h, 2); }
            }
        }
        if ((rc = upload(ctx, &p->d_rz_lut, lut.data(), lut.size())) != MJ_OK) return rc;
        a.lut = p->d_rz_lut;
    }
    // the un-resized pixels: a plan-owned buffer from the context's cache (64 bytes of slack: the kernels' 16-byte loads may
    // start before and end behind the bytes they use)
    p->src_bytes = p->info.rgb_bytes;
    MJ_HIP(ctx, ctx->cache.get((void **)&p->d_src, (size_t)p->src_bytes + 64));
    a.images = p->d_rz_images; a.tabs = p->d_rz_tabs; a.src = p->d_src;
    p->info.rgb_bytes = (int64_t)n_slots * out_image;
    p->info.total_pixels = (int64_t)n_slots * out_width * out_height;
    p->resized = true;
    guard.p = nullptr;
    *out = p;
    return MJ_OK;
}

}  // namespace
