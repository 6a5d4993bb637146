// Affine transform (mj_plan_request.affine): Pillow's Image.transform(img.size, Image.AFFINE, a, resample, fillcolor=fill) of every
// oriented image of the plan, in ONE launch between stage 2 (or the fused launch) and the resize launch.  It reads the plan's
// buffer of decoded pixels — stored order, the files' sizes — and writes, for every output, ONLY its window of the transformed
// image, densely, in the output's components, into a second plan-owned buffer which the resize launch then reads as upright
// images (resize_plan.hip: affine_stage).
//
// The arithmetic is Pillow's (tools/affine_model.py restates it; include/mijpeg.h has the rules): bilinear and bicubic evaluate
// the matrix at the pixel's centre in doubles, every operation rounded on its own (the library is compiled with
// -ffp-contract=off), and interpolate in doubles; NEAREST is either two host-built index tables (a1 == a3 == 0: Pillow finds the
// indices by accumulation) or closed-form 16.16 fixed point in wrapping 32-bit arithmetic (the sum Pillow accumulates is exact
// modulo 2^32).  A rule is evaluated at the window's ABSOLUTE coordinates: folding the origin into a2 / a5 gives other bits.
// transform_pixel is that arithmetic, once, for the kernel and for the host twin (mj_host_affine).
//
// Orientation costs no pass: the rules count in the oriented image, and the fetch maps an oriented coordinate to the stored one
// (tools/orient_model.py).  MJ_MODE_L on colour files converts every fetched tap before it is interpolated (convert, then
// transform); grey to RGB writes the one interpolated byte three times, and the fill's three bytes where the source lies outside.
//
// One thread per output pixel, all its components.  A workgroup takes kAffineTileSlow x kAffineTileFast pixels of one window, a
// wavefront every fourth row of them: 64 pixels along the layout's contiguous axis.  The reads are gathers through the caches (a
// rotated tile's footprint is a rotated rectangle); the finished bytes of a row go through LDS so that consecutive lanes store
// consecutive runs of 4 bytes (at any alignment) and never a byte outside the row.
//
// Perspective transform (mj_plan_request.perspective): Pillow's Image.transform(img.size, Image.PERSPECTIVE, c,
// resample, fillcolor=fill) in the same place, with the same launch geometry, fetch and 2 x 2 / 4 x 4 taps (k_perspective; records
// of its own, DevPerspectiveImage).  The coordinates are two IEEE double divisions per pixel (tools/perspective_model.py), NEAREST
// truncates them — no fixed point, no tables —, and a pixel whose coordinates are not inside the image, NaN and +-inf included, is
// fill: no double is converted to an int before it is known to lie in [0, w) x [0, h).  transform_pixel holds both launches'
// arithmetic (host twin: mj_host_perspective).
#include <math.h>

#include "plan.h"

namespace mj {

namespace {

// the components a tap has: colour to L converts where it fetches
template <int CS, int CO> struct TapComps { static constexpr int n = (CS == 3 && CO == 1) ? 1 : CS; };

// an oriented image in stored order: pixel (ox, oy) of the w x h oriented image out of the sw x sh stored one
template <int CS, int CO>
struct StoredFetch {
    const uint8_t *src;
    int sw, sh, w, h, obits;
    bool rowmajor;
    __host__ __device__ inline void operator()(int ox, int oy, unsigned *v) const {
        if (obits & 1) ox = w - 1 - ox;
        if (obits & 2) oy = h - 1 - oy;
        const int sx = (obits & 4) ? oy : ox, sy = (obits & 4) ? ox : oy;
        const uint8_t *p = src + (rowmajor ? (int64_t)sy * sw + sx : (int64_t)sx * sh + sy) * CS;
        if (CS == 3 && CO == 1) v[0] = mode_luma(p[0], p[1], p[2]);
        else
            for (int c = 0; c < CS; ++c) v[c] = p[c];
    }
};

__host__ __device__ inline int clipi(int v, int n) { return v < 0 ? 0 : v >= n ? n - 1 : v; }

__host__ __device__ inline double cubic(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2, p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

// What tells the two kinds of record apart where one function serves both
template <class Rec> struct IsPerspective { static constexpr bool value = false; };
template <> struct IsPerspective<DevPerspectiveImage> { static constexpr bool value = true; };

// Pixel (x, y) of the window of record im (window coordinates): out[CO] — the arithmetic of both launches, once, for the kernels
// and the host twins; the 2 x 2 and 4 x 4 taps are the same lines for both.  Every fetch is of a pixel inside the image: columns
// and rows are clipped or tested before they are read.
// A perspective record (tabs: unused): d is evaluated once (Pillow evaluates it twice: the same value), the two divisions are IEEE
// double divisions, and the inside test is written so that NaN and +-inf fail it.  No double becomes an int before it has passed
// that test: 0 / 0 — the one spot where Pillow's C is undefined — is fill.
template <int CS, int CO, class Rec, class Fetch>
__host__ __device__ inline void transform_pixel(const Rec &im, const int32_t *tabs, uint32_t fill, int x, int y, const Fetch &fetch, uint8_t *out) {
    constexpr bool kPerspective = IsPerspective<Rec>::value;
    constexpr int CV = TapComps<CS, CO>::n;
    const int X = x + im.x0, Y = y + im.y0, w = im.w, h = im.h;
    unsigned v[CV];
    bool inside = true;
    double xin = 0.0, yin = 0.0;
    if constexpr (kPerspective) {
        if (im.kind != 0) {
            const double xc = X + 0.5, yc = Y + 0.5;
            const double d = im.c[6] * xc + im.c[7] * yc + 1;
            xin = (im.c[0] * xc + im.c[1] * yc + im.c[2]) / d; yin = (im.c[3] * xc + im.c[4] * yc + im.c[5]) / d;
            inside = xin >= 0.0 && xin < w && yin >= 0.0 && yin < h;
        }
    }
    if (im.kind <= (kPerspective ? 1 : 2)) {
        int sx = X, sy = Y;
        if constexpr (kPerspective) {
            if (im.kind == 1) { sx = inside ? (int)xin : -1; sy = inside ? (int)yin : -1; }
        } else if (im.kind == 1) {
            sx = tabs[im.xtab + x]; sy = tabs[im.ytab + y];
        } else if (im.kind == 2) {
            const uint32_t ux = (uint32_t)im.fx[2] + (uint32_t)X * (uint32_t)im.fx[0] + (uint32_t)Y * (uint32_t)im.fx[1];
            const uint32_t uy = (uint32_t)im.fx[5] + (uint32_t)X * (uint32_t)im.fx[3] + (uint32_t)Y * (uint32_t)im.fx[4];
            sx = (int32_t)ux >> 16; sy = (int32_t)uy >> 16;
        }
        inside = sx >= 0 && sx < w && sy >= 0 && sy < h;
        if (inside) fetch(sx, sy, v);
    } else {
        if constexpr (!kPerspective) {
            const double xc = X + 0.5, yc = Y + 0.5;
            xin = im.a[0] * xc + im.a[1] * yc + im.a[2]; yin = im.a[3] * xc + im.a[4] * yc + im.a[5];
            inside = !(xin < 0.0 || xin >= w || yin < 0.0 || yin >= h);
        }
        if (inside) {
            xin -= 0.5; yin -= 0.5;
            const int ix = (int)floor(xin), iy = (int)floor(yin);
            const double dx = xin - ix, dy = yin - iy;
            if (im.kind == 3) {
                const int c0 = clipi(ix, w), c1 = clipi(ix + 1, w);
                unsigned p0[CV], p1[CV];
                double v1[CV], v2[CV];
                fetch(c0, clipi(iy, h), p0); fetch(c1, clipi(iy, h), p1);
                for (int c = 0; c < CV; ++c) v1[c] = (double)p0[c] + ((double)p1[c] - (double)p0[c]) * dx;
                if (iy + 1 >= 0 && iy + 1 < h) {
                    fetch(c0, iy + 1, p0); fetch(c1, iy + 1, p1);
                    for (int c = 0; c < CV; ++c) v2[c] = (double)p0[c] + ((double)p1[c] - (double)p0[c]) * dx;
                } else {
                    for (int c = 0; c < CV; ++c) v2[c] = v1[c];
                }
                for (int c = 0; c < CV; ++c) v[c] = (unsigned)(int)(v1[c] + (v2[c] - v1[c]) * dy);
            } else {
                const int c0 = clipi(ix - 1, w), c1 = clipi(ix, w), c2 = clipi(ix + 1, w), c3 = clipi(ix + 2, w);
                double r[4][CV];
                for (int k = 0; k < 4; ++k) {
                    const int row = iy - 1 + k;
                    if (k == 0 || (row >= 0 && row < h)) {
                        const int rr = k == 0 ? clipi(row, h) : row;
                        unsigned p0[CV], p1[CV], p2[CV], p3[CV];
                        fetch(c0, rr, p0); fetch(c1, rr, p1); fetch(c2, rr, p2); fetch(c3, rr, p3);
                        for (int c = 0; c < CV; ++c) r[k][c] = cubic((double)p0[c], (double)p1[c], (double)p2[c], (double)p3[c], dx);
                    } else {
                        for (int c = 0; c < CV; ++c) r[k][c] = r[k - 1][c];
                    }
                }
                for (int c = 0; c < CV; ++c) {
                    const double t = cubic(r[0][c], r[1][c], r[2][c], r[3][c], dy);
                    v[c] = t <= 0.0 ? 0u : t >= 255.0 ? 255u : (unsigned)(int)t;
                }
            }
        }
    }
    for (int c = 0; c < CO; ++c) out[c] = inside ? (uint8_t)v[CV == 1 ? 0 : c] : (uint8_t)(fill >> (8 * c));
}

template <int CS, int CO>
__global__ __launch_bounds__(256) void k_affine(const AffineArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * kAffineTileFast * CO];
    const int tiles = a.tiles_slow * a.tiles_fast;
    const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;      // (launch_affine: the grid's tail is idle)
    if (wg >= (int64_t)a.n_images * tiles) return;
    const int img = (int)(wg / tiles), t = (int)(wg - (int64_t)img * tiles);
    const int ts = t / a.tiles_fast, tf = t - ts * a.tiles_fast;
    const DevAffineImage im = a.images[img];
    const bool rowmajor = (a.layout & 1) != 0;
    const int nfast = rowmajor ? im.win_w : im.win_h, nslow = rowmajor ? im.win_h : im.win_w;
    const int f0 = tf * kAffineTileFast, s0 = ts * kAffineTileSlow;
    if (f0 >= nfast || s0 >= nslow) return;       // (a window smaller than the plan's largest)
    const int s1 = min(s0 + kAffineTileSlow, nslow), ne = (min(f0 + kAffineTileFast, nfast) - f0) * CO;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, f = f0 + lane;
    unsigned char *ostage = smem + wave * (kAffineTileFast * CO);
    const StoredFetch<CS, CO> fetch{a.src + im.src_off, im.sw, im.sh, im.w, im.h, im.obits, rowmajor};
    unsigned char *dst = a.dst + im.dst_off;
    for (int s = s0 + wave; s < s1; s += 4) {
        if (f < nfast) {
            uint8_t px[CO];
            transform_pixel<CS, CO>(im, a.tabs, a.fill, rowmajor ? f : s, rowmajor ? s : f, fetch, px);
#pragma unroll
            for (int c = 0; c < CO; ++c) ostage[lane * CO + c] = px[c];
        }
        // (the staging row is this wavefront's own: its lanes only have to see each other's LDS writes)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        unsigned char *orow = dst + ((int64_t)s * nfast + f0) * CO;
        const int b0 = 4 * lane;
        if (b0 + 4 <= ne) {
            const unsigned word = *reinterpret_cast<const unsigned *>(ostage + b0);
            __builtin_memcpy(orow + b0, &word, 4);            // (rows start at any alignment)
        } else {
            for (int b = b0; b < ne; ++b) orow[b] = ostage[b];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// The same launch for the records of a perspective transform.  (The body is k_affine's, repeated: one shared body, inlined into
// both, changed the scalar loads of the four k_affine instances, which are to stay the instructions they were.)
template <int CS, int CO>
__global__ __launch_bounds__(256) void k_perspective(const PerspectiveArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * kAffineTileFast * CO];
    const int tiles = a.tiles_slow * a.tiles_fast;
    const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;      // (launch_perspective: the grid's tail is idle)
    if (wg >= (int64_t)a.n_images * tiles) return;
    const int img = (int)(wg / tiles), t = (int)(wg - (int64_t)img * tiles);
    const int ts = t / a.tiles_fast, tf = t - ts * a.tiles_fast;
    const DevPerspectiveImage im = a.images[img];
    const bool rowmajor = (a.layout & 1) != 0;
    const int nfast = rowmajor ? im.win_w : im.win_h, nslow = rowmajor ? im.win_h : im.win_w;
    const int f0 = tf * kAffineTileFast, s0 = ts * kAffineTileSlow;
    if (f0 >= nfast || s0 >= nslow) return;       // (a window smaller than the plan's largest)
    const int s1 = min(s0 + kAffineTileSlow, nslow), ne = (min(f0 + kAffineTileFast, nfast) - f0) * CO;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, f = f0 + lane;
    unsigned char *ostage = smem + wave * (kAffineTileFast * CO);
    const StoredFetch<CS, CO> fetch{a.src + im.src_off, im.sw, im.sh, im.w, im.h, im.obits, rowmajor};
    unsigned char *dst = a.dst + im.dst_off;
    for (int s = s0 + wave; s < s1; s += 4) {
        if (f < nfast) {
            uint8_t px[CO];
            transform_pixel<CS, CO>(im, nullptr, a.fill, rowmajor ? f : s, rowmajor ? s : f, fetch, px);
#pragma unroll
            for (int c = 0; c < CO; ++c) ostage[lane * CO + c] = px[c];
        }
        // (the staging row is this wavefront's own: its lanes only have to see each other's LDS writes)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        unsigned char *orow = dst + ((int64_t)s * nfast + f0) * CO;
        const int b0 = 4 * lane;
        if (b0 + 4 <= ne) {
            const unsigned word = *reinterpret_cast<const unsigned *>(ostage + b0);
            __builtin_memcpy(orow + b0, &word, 4);            // (rows start at any alignment)
        } else {
            for (int b = b0; b < ne; ++b) orow[b] = ostage[b];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

template <int CS, int CO>
void affine_host_t(const uint8_t *src, const DevAffineImage &im, const int32_t *tabs, uint32_t fill, uint8_t *out) {
    const StoredFetch<CS, CO> fetch{src, im.sw, im.sh, im.w, im.h, im.obits, true};
    for (int y = 0; y < im.win_h; ++y)
        for (int x = 0; x < im.win_w; ++x) transform_pixel<CS, CO>(im, tabs, fill, x, y, fetch, out + ((int64_t)y * im.win_w + x) * CO);
}

template <int CS, int CO>
void perspective_host_t(const uint8_t *src, const DevPerspectiveImage &im, uint32_t fill, uint8_t *out) {
    const StoredFetch<CS, CO> fetch{src, im.sw, im.sh, im.w, im.h, im.obits, true};
    for (int y = 0; y < im.win_h; ++y)
        for (int x = 0; x < im.win_w; ++x) transform_pixel<CS, CO>(im, nullptr, fill, x, y, fetch, out + ((int64_t)y * im.win_w + x) * CO);
}

// one workgroup per tile, as launch_resize numbers them
dim3 tile_grid(int n_images, int tiles_slow, int tiles_fast) {
    const int64_t total = (int64_t)n_images * tiles_slow * tiles_fast, gx = std::min<int64_t>(total, kResizeGridX);
    return dim3((unsigned)gx, (unsigned)((total + gx - 1) / gx));
}

}  // namespace

const char *perspective_fault(const double *c, int filter, int w, int h) {
    if (filter != MJ_AFFINE_NEAREST && filter != MJ_AFFINE_BILINEAR && filter != MJ_AFFINE_BICUBIC) return "the filter is none of MJ_AFFINE_*";
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(c[k])) return "a coefficient is not finite";
    if (w >= 32768 || h >= 32768) return "an image with a side of 32768 or more";
    return nullptr;
}

int perspective_kind(int filter) { return filter == MJ_AFFINE_NEAREST ? 1 : filter == MJ_AFFINE_BILINEAR ? 3 : 4; }

void perspective_host(const uint8_t *src, const DevPerspectiveImage &im, int ncomp, int out_ncomp, uint32_t fill, uint8_t *out) {
    if (ncomp == 3 && out_ncomp == 1) perspective_host_t<3, 1>(src, im, fill, out);
    else if (ncomp == 3) perspective_host_t<3, 3>(src, im, fill, out);
    else if (out_ncomp == 3) perspective_host_t<1, 3>(src, im, fill, out);
    else perspective_host_t<1, 1>(src, im, fill, out);
}

hipError_t launch_perspective(hipStream_t stream, const PerspectiveArgs &a, int ncomp, int out_ncomp) {
    if (a.n_images <= 0) return hipSuccess;
    const dim3 grid = tile_grid(a.n_images, a.tiles_slow, a.tiles_fast), block(256);
    if (ncomp == 3 && out_ncomp == 1) hipLaunchKernelGGL((k_perspective<3, 1>), grid, block, 0, stream, a);
    else if (ncomp == 3) hipLaunchKernelGGL((k_perspective<3, 3>), grid, block, 0, stream, a);
    else if (out_ncomp == 3) hipLaunchKernelGGL((k_perspective<1, 3>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((k_perspective<1, 1>), grid, block, 0, stream, a);
    return hipGetLastError();
}

const char *affine_fault(const double *a, int filter, int w, int h) {
    if (filter != MJ_AFFINE_NEAREST && filter != MJ_AFFINE_BILINEAR && filter != MJ_AFFINE_BICUBIC) return "the filter is none of MJ_AFFINE_*";
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(a[k])) return "a matrix entry is not finite";
    if (w >= 32768 || h >= 32768) return "an image with a side of 32768 or more";
    // the corner pixels' centres, and under NEAREST the corners Pillow's check_fixed tests
    for (int pass = 0; pass < (filter == MJ_AFFINE_NEAREST ? 2 : 1); ++pass)
        for (int k = 0; k < 4; ++k) {
            const double x = pass ? ((k & 1) ? (double)w : 0.0) : ((k & 1) ? w - 0.5 : 0.5), y = pass ? ((k & 2) ? (double)h : 0.0) : ((k & 2) ? h - 0.5 : 0.5);
            if (!(fabs(a[0] * x + a[1] * y + a[2]) < 32768.0) || !(fabs(a[3] * x + a[4] * y + a[5]) < 32768.0))
                return "a corner of the output has a source coordinate of magnitude 32768 or more";
        }
    if (filter == MJ_AFFINE_NEAREST && !(a[1] == 0 && a[3] == 0)) {
        const double fixed[6] = {a[0], a[1], a[2] + a[0] * 0.5 + a[1] * 0.5, a[3], a[4], a[5] + a[3] * 0.5 + a[4] * 0.5};
        for (int k = 0; k < 6; ++k)
            if (!(fabs(fixed[k]) < 32767.0)) return "a matrix entry of magnitude 32767 or more does not fit NEAREST's 16.16 fixed point";
    }
    return nullptr;
}

int affine_kind(const double *a, int filter) {
    if (filter == MJ_AFFINE_NEAREST) return a[1] == 0 && a[3] == 0 ? 1 : 2;
    return filter == MJ_AFFINE_BILINEAR ? 3 : 4;
}

void affine_fixed(const double *a, int32_t fx[6]) {
    auto fix = [](double v) { return (int32_t)floor(v * 65536.0 + 0.5); };
    fx[0] = fix(a[0]); fx[1] = fix(a[1]); fx[3] = fix(a[3]); fx[4] = fix(a[4]);
    fx[2] = fix(a[2] + a[0] * 0.5 + a[1] * 0.5);
    fx[5] = fix(a[5] + a[3] * 0.5 + a[4] * 0.5);
}

void affine_scale_table(double scale, double offset, int size, int first, int n, int32_t *out) {
    double o = offset + scale * 0.5;
    for (int j = 0; j < first + n; ++j) {
        const int idx = o < 0.0 ? -1 : (int)o;
        if (j >= first) out[j - first] = idx >= 0 && idx < size ? idx : -1;
        o += scale;
    }
}

void affine_host(const uint8_t *src, const DevAffineImage &im, const int32_t *tabs, int ncomp, int out_ncomp, uint32_t fill, uint8_t *out) {
    if (ncomp == 3 && out_ncomp == 1) affine_host_t<3, 1>(src, im, tabs, fill, out);
    else if (ncomp == 3) affine_host_t<3, 3>(src, im, tabs, fill, out);
    else if (out_ncomp == 3) affine_host_t<1, 3>(src, im, tabs, fill, out);
    else affine_host_t<1, 1>(src, im, tabs, fill, out);
}

hipError_t launch_affine(hipStream_t stream, const AffineArgs &a, int ncomp, int out_ncomp) {
    if (a.n_images <= 0) return hipSuccess;
    const dim3 grid = tile_grid(a.n_images, a.tiles_slow, a.tiles_fast), block(256);
    if (ncomp == 3 && out_ncomp == 1) hipLaunchKernelGGL((k_affine<3, 1>), grid, block, 0, stream, a);
    else if (ncomp == 3) hipLaunchKernelGGL((k_affine<3, 3>), grid, block, 0, stream, a);
    else if (out_ncomp == 3) hipLaunchKernelGGL((k_affine<1, 3>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((k_affine<1, 1>), grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace mj

extern "C" {

int mj_host_affine(const uint8_t *src, int32_t w, int32_t h, int32_t ncomp, const double *a, int32_t filter, const uint8_t *fill, int32_t x0, int32_t y0,
                   int32_t win_w, int32_t win_h, uint8_t *out) {
    if (!src || !a || !out || w < 1 || h < 1 || (ncomp != 1 && ncomp != 3)) return MJ_ERR_INVALID;
    // (the window may reach beyond the source's size: Image.transform(size, ..) with a size of its own is the window (0, 0, size))
    if (win_w < 1 || win_h < 1 || x0 < 0 || y0 < 0 || (int64_t)x0 + win_w >= 32768 || (int64_t)y0 + win_h >= 32768) return MJ_ERR_INVALID;
    if (w >= 32768 || h >= 32768 || mj::affine_fault(a, filter, std::max(w, x0 + win_w), std::max(h, y0 + win_h))) return MJ_ERR_INVALID;
    mj::DevAffineImage im{};
    im.sw = im.w = w; im.sh = im.h = h;
    im.x0 = x0; im.y0 = y0; im.win_w = win_w; im.win_h = win_h;
    im.kind = mj::affine_kind(a, filter);
    for (int k = 0; k < 6; ++k) im.a[k] = a[k];
    std::vector<int32_t> tabs((size_t)win_w + win_h);
    if (im.kind == 1) {
        im.xtab = 0; im.ytab = win_w;
        mj::affine_scale_table(a[0], a[2], w, x0, win_w, tabs.data());
        mj::affine_scale_table(a[4], a[5], h, y0, win_h, tabs.data() + win_w);
    } else if (im.kind == 2) {
        mj::affine_fixed(a, im.fx);
    }
    uint32_t f = 0;
    for (int c = 0; c < ncomp && fill; ++c) f |= (uint32_t)fill[c] << (8 * c);
    mj::affine_host(src, im, tabs.data(), ncomp, ncomp, f, out);
    return MJ_OK;
}

int mj_host_perspective(const uint8_t *src, int32_t w, int32_t h, int32_t ncomp, const double *c, int32_t filter, const uint8_t *fill, int32_t x0,
                        int32_t y0, int32_t win_w, int32_t win_h, uint8_t *out) {
    if (!src || !c || !out || w < 1 || h < 1 || (ncomp != 1 && ncomp != 3)) return MJ_ERR_INVALID;
    // (the window may reach beyond the source's size, as mj_host_affine's may)
    if (win_w < 1 || win_h < 1 || x0 < 0 || y0 < 0 || (int64_t)x0 + win_w >= 32768 || (int64_t)y0 + win_h >= 32768) return MJ_ERR_INVALID;
    if (mj::perspective_fault(c, filter, w, h)) return MJ_ERR_INVALID;
    mj::DevPerspectiveImage im{};
    im.sw = im.w = w; im.sh = im.h = h;
    im.x0 = x0; im.y0 = y0; im.win_w = win_w; im.win_h = win_h;
    im.kind = mj::perspective_kind(filter);
    for (int k = 0; k < 8; ++k) im.c[k] = c[k];
    uint32_t f = 0;
    for (int k = 0; k < ncomp && fill; ++k) f |= (uint32_t)fill[k] << (8 * k);
    mj::perspective_host(src, im, ncomp, ncomp, f, out);
    return MJ_OK;
}

}  // extern "C"
