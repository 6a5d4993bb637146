// Two-step resize (mj_plan_request.reducing_gap): the first step, Pillow's Image.reduce((fx, fy)) of every image of the plan in
// ONE launch between stage 2 (or the fused launch) and the resize launch.  It reads the plan's buffer of decoded pixels at the
// files' sizes and writes a second plan-owned buffer of reduced images, packed, which the resize launch then reads as it reads
// the first (its tables are built for the reduced sizes and the fractional box, resize_plan.hip: reduce_stage).
//
// The arithmetic is Pillow's (tools/reduce_model.py restates it): a cell of n pixels becomes ((sum + n / 2) * m(n)) >> 24 per
// component in 32-bit unsigned arithmetic, m(n) = (uint32)(float32(2^32) / float32(256 n)); partial cells at an edge use their
// own n.  The host evaluates m(n) and n / 2 for the four kinds of cell an image has — the kernel never divides a sum — and
// refuses cells above 65536 pixels, so sums stay below 2^24 and products inside 32 bits.
//
// One kernel body serves both layouts: an image is rows x len pixels of C interleaved bytes (row-major: H x W; x-major: W x H),
// the factors are (f_slow, f_fast), and a 2-D sum with one rounding does not care which axis is which.  Orientation is free: an
// axis the orientation reverses has its cell boundaries at size mod f + k * f (DevReduceImage::off_*), so the reduced stored-order
// image is the stored-order counterpart of Pillow's reduced oriented image and the resize's oriented instances run on it unchanged.
//
// A workgroup takes tile_slow reduced rows x tile_fast reduced pixels of one image; each wavefront every fourth reduced row.  Rows
// start at any byte alignment (the pitch is len * C — for a view of a decoded image, mj_plan_request.views, that image's row:
// DevReduceImage::pitch), so — as the resize's row-major width pass — a wavefront stages a source row
// segment in LDS with aligned 16-byte loads (they may begin up to 15 bytes before and end up to 15 behind the bytes used: inside
// the buffer's slack) and its lanes gather their cells from there, f_slow rows one after the other into 32-bit registers.  A
// segment longer than the staging row goes in pieces.  The finished bytes of a reduced row go through LDS once more, so that
// consecutive lanes store consecutive runs of 8 bytes (at any alignment) and never a byte outside the row.
// MODE_L on colour files: Pillow converts before it reduces, so the LUMA instance applies mode_luma to every pixel it reads and
// writes one component; the resize launch of such a plan is the plain one-component one.
#include "plan.h"

namespace mj {

void reduce_factors(int src_w, int src_h, int dst_w, int dst_h, double gap, int *fx, int *fy) {
    const int x = (int)((double)src_w / (double)dst_w / gap), y = (int)((double)src_h / (double)dst_h / gap);
    *fx = x > 1 ? x : 1;
    *fy = y > 1 ? y : 1;
}

uint32_t reduce_multiplier(uint32_t n) {
    volatile float top = 4294967296.0f, bottom = (float)(256u * n);      // (256 n <= 2^24: exact)
    volatile float q = top / bottom;
    return (uint32_t)q;
}

void reduce_record(int rows, int len, int f_slow, int f_fast, int phase_slow, int phase_fast, DevReduceImage *out) {
    out->rows = rows; out->len = out->pitch = len;
    out->f_slow = f_slow; out->f_fast = f_fast;
    out->off_slow = phase_slow ? f_slow - phase_slow : 0;
    out->off_fast = phase_fast ? f_fast - phase_fast : 0;
    // (an axis without a partial cell: its entry is never looked up)
    const uint32_t ps = rows % f_slow ? rows % f_slow : f_slow, pf = len % f_fast ? len % f_fast : f_fast;
    for (int kind = 0; kind < 4; ++kind) {
        const uint32_t n = ((kind & 2) ? ps : (uint32_t)f_slow) * ((kind & 1) ? pf : (uint32_t)f_fast);
        out->mul[kind] = reduce_multiplier(n);
        out->half[kind] = n / 2;
    }
}

void reduce_host(const uint8_t *src, const DevReduceImage &im, int ncomp, bool luma, uint8_t *out) {
    const int CO = luma ? 1 : ncomp;
    const int orows = (im.rows + im.f_slow - 1) / im.f_slow, olen = (im.len + im.f_fast - 1) / im.f_fast;
    for (int r = 0; r < orows; ++r) {
        const int ys = std::max(0, r * im.f_slow - im.off_slow), ye = (int)std::min<int64_t>(im.rows, (int64_t)(r + 1) * im.f_slow - im.off_slow);
        for (int p = 0; p < olen; ++p) {
            const int c0 = std::max(0, p * im.f_fast - im.off_fast), c1 = (int)std::min<int64_t>(im.len, (int64_t)(p + 1) * im.f_fast - im.off_fast);
            const int kind = ((ye - ys) != im.f_slow ? 2 : 0) | ((c1 - c0) != im.f_fast ? 1 : 0);
            for (int c = 0; c < CO; ++c) {
                uint32_t acc = 0;
                for (int y = ys; y < ye; ++y)
                    for (int x = c0; x < c1; ++x) {
                        const uint8_t *s = src + ((int64_t)y * im.pitch + x) * ncomp;
                        acc += luma ? mode_luma(s[0], s[1], s[2]) : s[c];
                    }
                out[((int64_t)r * olen + p) * CO + c] = (uint8_t)(((acc + im.half[kind]) * im.mul[kind]) >> 24);
            }
        }
    }
}

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int kReduceLaneElems = 8;      // reduced bytes of a row per lane: a tile's row has at most 64 * 8 of them (16: 176 registers)
constexpr int kReduceOutRow = 64 * kReduceLaneElems;

template <int CS, bool LUMA>
__global__ __launch_bounds__(256) void k_reduce(const ReduceArgs a) {
    constexpr int CO = LUMA ? 1 : CS;
    constexpr int kPiece = (kReduceStage - 16) / CS;       // source pixels staged at a time: 15 + 16 * ... stays inside the row
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * (kReduceStage + kReduceOutRow)];
    const int tiles = a.tiles_slow * a.tiles_fast;
    const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;      // (launch_reduce: the grid's tail is idle)
    if (wg >= (int64_t)a.n_images * tiles) return;
    const int img = (int)(wg / tiles), t = (int)(wg - (int64_t)img * tiles);
    const int ts = t / a.tiles_fast, tf = t - ts * a.tiles_fast;
    const DevReduceImage im = a.images[img];
    const int orows = (im.rows + im.f_slow - 1) / im.f_slow, olen = (im.len + im.f_fast - 1) / im.f_fast;
    const int r0 = ts * a.tile_slow, p0 = tf * a.tile_fast;
    if (r0 >= orows || p0 >= olen) return;       // (an image smaller than the batch's largest)
    const int r1 = min(r0 + a.tile_slow, orows), p1 = min(p0 + a.tile_fast, olen);
    const int ne = (p1 - p0) * CO;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    unsigned char *stage = smem + wave * kReduceStage, *ostage = smem + 4 * kReduceStage + wave * kReduceOutRow;
    const unsigned char *src = a.src + im.src_off;
    unsigned char *dst = a.dst + im.dst_off;
    // the source pixels of a row the tile's cells cover
    const int xs = max(0, p0 * im.f_fast - im.off_fast), xe = min(im.len, p1 * im.f_fast - im.off_fast);
    // this lane's elements e = lane + 64 k: their cells along the row, and component
    int c0[kReduceLaneElems], c1[kReduceLaneElems], comp[kReduceLaneElems];
#pragma unroll
    for (int k = 0; k < kReduceLaneElems; ++k) {
        const int e = lane + 64 * k, pix = e / CO;
        comp[k] = e - pix * CO;
        c0[k] = max(0, (p0 + pix) * im.f_fast - im.off_fast);
        c1[k] = e < ne ? min(im.len, (p0 + pix + 1) * im.f_fast - im.off_fast) : c0[k];      // (no such element: an empty cell)
    }
    for (int r = r0 + wave; r < r1; r += 4) {
        const int ys = max(0, r * im.f_slow - im.off_slow), ye = min(im.rows, (r + 1) * im.f_slow - im.off_slow);
        unsigned acc[kReduceLaneElems];
#pragma unroll
        for (int k = 0; k < kReduceLaneElems; ++k) acc[k] = 0u;
        for (int y = ys; y < ye; ++y) {
            for (int px = xs; px < xe; px += kPiece) {
                const int pe = min(px + kPiece, xe);
                const unsigned char *row = src + ((int64_t)y * im.pitch + px) * CS;
                const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 15);
                const u32x4 *p = reinterpret_cast<const u32x4 *>(row - mis);
                const int n16 = (mis + (pe - px) * CS + 15) >> 4;          // <= kReduceStage / 16
                for (int j = lane; j < n16; j += 64) reinterpret_cast<u32x4 *>(stage)[j] = p[j];
                // (the staging row is this wavefront's own: its lanes only have to see each other's LDS writes)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int k = 0; k < kReduceLaneElems; ++k) {
                    const int q0 = max(c0[k], px), q1 = min(c1[k], pe);
                    const unsigned char *s = stage + mis + (q0 - px) * CS + comp[k];
                    for (int q = q0; q < q1; ++q, s += CS) {
                        if constexpr (LUMA) acc[k] += mode_luma(s[0], s[1], s[2]);
                        else acc[k] += s[0];
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
        const int kind_slow = (ye - ys) != im.f_slow ? 2 : 0;
        unsigned char *orow = dst + ((int64_t)r * olen + p0) * CO;
        // the finished bytes through LDS, so that a lane stores 8 consecutive ones (single bytes cost a store each: measured, the
        // launch took as long as its output was large)
#pragma unroll
        for (int k = 0; k < kReduceLaneElems; ++k) {
            // (selected, not indexed: the record stays in registers)
            const bool part = (c1[k] - c0[k]) != im.f_fast;
            const unsigned mul = kind_slow ? (part ? im.mul[3] : im.mul[2]) : (part ? im.mul[1] : im.mul[0]);
            const unsigned half = kind_slow ? (part ? im.half[3] : im.half[2]) : (part ? im.half[1] : im.half[0]);
            ostage[lane + 64 * k] = (unsigned char)(((acc[k] + half) * mul) >> 24);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int b0 = kReduceLaneElems * lane;
        if (b0 + kReduceLaneElems <= ne) {
            const uint2 v = *reinterpret_cast<const uint2 *>(ostage + b0);
            __builtin_memcpy(orow + b0, &v, kReduceLaneElems);            // (rows start at any alignment)
        } else {
            for (int b = b0; b < ne; ++b) orow[b] = ostage[b];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

}  // namespace

hipError_t launch_reduce(hipStream_t stream, const ReduceArgs &a, int ncomp, bool luma) {
    if (a.n_images <= 0) return hipSuccess;
    // one workgroup per tile, as launch_resize numbers them
    const int64_t total = (int64_t)a.n_images * a.tiles_slow * a.tiles_fast, gx = std::min<int64_t>(total, kResizeGridX);
    const dim3 grid((unsigned)gx, (unsigned)((total + gx - 1) / gx)), block(256);
    if (luma) hipLaunchKernelGGL((k_reduce<3, true>), grid, block, 0, stream, a);
    else if (ncomp == 3) hipLaunchKernelGGL((k_reduce<3, false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((k_reduce<1, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}

// the tile of a reducing plan's launch (resize_plan.hip: reduce_stage): a row of at most 64 * kReduceLaneElems reduced bytes
int reduce_tile_fast(int out_ncomp) { return kReduceOutRow / out_ncomp; }

// the source pixels of a row a wavefront stages at a time, k_reduce<CS, ...>'s kPiece (mj_debug_reduce_launch reports it)
int reduce_piece(int src_ncomp) { return (kReduceStage - 16) / src_ncomp; }

}  // namespace mj

extern "C" {

int mj_host_reduce_factors(int32_t src_w, int32_t src_h, int32_t dst_w, int32_t dst_h, double gap, int32_t *fx, int32_t *fy) {
    if (!fx || !fy || src_w < 1 || src_h < 1 || dst_w < 1 || dst_h < 1 || src_w > 65535 || src_h > 65535 || dst_w > 65535 || dst_h > 65535 ||
        !std::isfinite(gap) || !(gap >= 1.0))
        return MJ_ERR_INVALID;
    int x, y;
    mj::reduce_factors(src_w, src_h, dst_w, dst_h, gap, &x, &y);
    *fx = x; *fy = y;
    return MJ_OK;
}

int mj_host_reduce(const uint8_t *src, int32_t w, int32_t h, int32_t ncomp, int32_t fx, int32_t fy, int32_t phase_x, int32_t phase_y, uint8_t *out) {
    if (!src || !out || w < 1 || h < 1 || w > 65535 || h > 65535 || (ncomp != 1 && ncomp != 3) || fx < 1 || fy < 1 ||
        (int64_t)fx * fy > mj::kReduceMaxCell)
        return MJ_ERR_INVALID;
    // (a phase is what a reversed axis has: 0, or size mod f)
    if ((phase_x != 0 && phase_x != w % fx) || (phase_y != 0 && phase_y != h % fy)) return MJ_ERR_INVALID;
    mj::DevReduceImage im{};
    mj::reduce_record(h, w, fy, fx, phase_y, phase_x, &im);
    mj::reduce_host(src, im, ncomp, false, out);
    return MJ_OK;
}

}  // extern "C"
