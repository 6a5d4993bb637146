// EXIF orientation at the files' own sizes: an oriented plan (mj_plan_request.orientations, no size) decodes into a plan-owned buffer in
// stored order, as a resized plan does, and ONE launch over all its images writes every image oriented into its packed place
// in the output.  tools/orient_model.py is the definition: the eight values are a transpose (5..8) followed by reversed
// columns and / or rows.
//
// In memory an image is rows x len pixels, len along the contiguous axis (row-major plans: height x width; x-major plans:
// width x height), and an orientation is three bits on that array (DevOrientImage::op): the destination's rows backwards,
// its contiguous axis backwards, rows and columns exchanged.  A workgroup takes one 64 x 64 pixel tile of the source:
//   in   16-byte loads along the source's contiguous axis (at whatever alignment the tile starts: up to 15 bytes behind the
//        tile's row are read along, which lie in the row, the next image or the buffer's slack) into LDS rows
//   out  consecutive lanes store consecutive bytes of a destination row — whole runs of 64 pixels along the destination's
//        contiguous axis, the source read backwards for a reversed axis and down an LDS column for orientations 5..8.
// The LDS row pitch is 64 * C + 4 bytes = 49 dwords (colour) or 17 (grey): odd, so that the lanes of a column read — one
// row apart each — fall into different banks instead of all into one.  Planar plans read the same interleaved source and
// store one plane after the other.
//
// Output colour mode (mj_plan_request.mode, no size): k_orient<CS, CO> with CS != CO is the same launch converting on its way — the tile
// lies in LDS in the source's components, the store loop runs over the output's: a grey byte goes into all three components,
// a colour pixel becomes its L (mode_luma).  Such a plan has the launch for upright images too (op 0: a copy that converts), and
// an image's place in the output is no longer its place in the source (dst_off: the same pixels, CO components each).
#include "plan.h"

namespace mj {
constexpr int kTile = 64;
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));


template <int C, int CO = C>
__global__ __launch_bounds__(256) void k_orient(const OrientArgs a) {
    constexpr int P = kTile * C + 4;
    __shared__ __attribute__((aligned(16))) unsigned char T[kTile * P];
    const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;      // (launch_orient: the grid's tail is idle)
    if (wg >= a.total_tiles) return;
    int img = 0, hi = a.n_images - 1;
    while (img < hi) {                                                    // the last image whose first tile is not behind wg
        const int mid = (img + hi + 1) >> 1;
        if (a.tile_prefix[mid] <= wg) img = mid; else hi = mid - 1;
    }
    const DevOrientImage im = a.images[img];
    const int t = (int)(wg - a.tile_prefix[img]);
    const int tr = t / im.tiles_l, tl = t - tr * im.tiles_l;
    const int r0 = tr * kTile, l0 = tl * kTile;
    const int nr = min(kTile, im.rows - r0), nl = min(kTile, im.len - l0);
    const int tid = threadIdx.x;
    const unsigned char *src = a.src + im.src_off + ((int64_t)r0 * im.len + l0) * C;
    const int nch = (nl * C + 15) >> 4;
    for (int i = tid; i < nr * nch; i += 256) {
        const int row = i / nch, j = i - row * nch;
        u32x4 v;
        __builtin_memcpy(&v, src + (int64_t)row * im.len * C + 16 * j, 16);
        unsigned *d = reinterpret_cast<unsigned *>(T + row * P + 16 * j);
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
    __syncthreads();
    const bool swap = (im.op & 4) != 0, back_r = (im.op & 1) != 0, back_l = (im.op & 2) != 0;
    // the destination: drows x dlen pixels; this tile's part of it is ndr x ndl, first pixel (dr0, dl0)
    const int drows = swap ? im.len : im.rows, dlen = swap ? im.rows : im.len;
    const int ndr = swap ? nl : nr, ndl = swap ? nr : nl;
    const int sr0 = swap ? l0 : r0, sl0 = swap ? r0 : l0;
    const int dr0 = back_r ? drows - (sr0 + ndr) : sr0, dl0 = back_l ? dlen - (sl0 + ndl) : sl0;
    unsigned char *dst = a.dst + im.dst_off;
    const bool planar = a.planar != 0 && CO > 1;
    const int total = ndr * ndl * CO;
    for (int i = tid; i < total; i += 256) {
        int dr, dl, c;
        if (planar) { c = i / (ndr * ndl); const int rem = i - c * (ndr * ndl); dr = rem / ndl; dl = rem - dr * ndl; }
        else { dr = i / (ndl * CO); const int e = i - dr * (ndl * CO); dl = e / CO; c = e - dl * CO; }
        const int ar = back_r ? ndr - 1 - dr : dr, al = back_l ? ndl - 1 - dl : dl;
        const unsigned char *s = T + (swap ? al : ar) * P + (swap ? ar : al) * C;
        unsigned char v;
        if constexpr (C == CO) v = s[c];
        else if constexpr (C == 1) v = s[0];                                    // grey into every component
        else v = (unsigned char)mode_luma(s[0], s[1], s[2]);                    // colour to L
        const int64_t pix = (int64_t)(dr0 + dr) * dlen + dl0 + dl;
        if (planar) dst[(int64_t)c * drows * dlen + pix] = v;
        else dst[pix * CO + c] = v;
    }
}

}  // namespace

hipError_t launch_orient(hipStream_t stream, const OrientArgs &a, int ncomp, int out_ncomp) {
    if (a.n_images <= 0 || a.total_tiles <= 0) return hipSuccess;
    const int64_t gx = std::min<int64_t>(a.total_tiles, kResizeGridX);
    const dim3 grid((unsigned)gx, (unsigned)((a.total_tiles + gx - 1) / gx)), block(256);
    if (out_ncomp && out_ncomp != ncomp) {
        if (ncomp == 3) hipLaunchKernelGGL((k_orient<3, 1>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((k_orient<1, 3>), grid, block, 0, stream, a);
    } else if (ncomp == 3) hipLaunchKernelGGL(k_orient<3>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(k_orient<1>, grid, block, 0, stream, a);
    return hipGetLastError();
}

// The plan of a normalised request without a size that has orientations (not all upright) or a mode (not the batch's own): one
// that converts has the launch for upright images too.
int create_oriented(const PlanRequest &q) {
    const char *fn = kCreateFn;
    mj_context *ctx = q.ctx; const mj_batch *b = q.b; mj_plan **out = q.out;
    const mj_roi *rois = q.r.rois; const uint8_t *orientations = q.r.orientations; const int mode = q.r.mode;
    if (!b->images) return fail(ctx, MJ_ERR_INVALID, "%s: NULL argument", fn);
    std::vector<mj_roi> stored;
    if (rois)
        if (int rc = stored_windows(q, rois, stored)) return rc;
    mj_plan *p = nullptr;
    if (int rc = mj::plan_create_common(ctx, b, rois ? stored.data() : nullptr, rois != nullptr, &p)) return rc;
    PlanGuard guard{p};
    const int n = p->n_images, C = p->ncomp, CO = mode ? mode : C;
    const bool xmajor = (p->layout & 1) == 0;
    std::vector<mj::DevOrientImage> oi((size_t)n);
    std::vector<int64_t> prefix((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) {
        const int w = p->windowed ? p->h_win[i].w : p->h_images[i].width, h = p->windowed ? p->h_win[i].h : p->h_images[i].height;
        const int bits = orientations ? mj::orient_bits(orientations[i]) : 0;
        const int fx = bits & 1, fy = (bits >> 1) & 1;
        mj::DevOrientImage &o = oi[(size_t)i];
        o.src_off = p->h_images[i].rgb_off;
        o.dst_off = o.src_off / C * CO;       // (the packing counts pixels: the same ones, CO components each)
        if (mode) p->h_out_off.push_back(o.dst_off);
        o.rows = xmajor ? w : h; o.len = xmajor ? h : w;
        o.tiles_l = (o.len + mj::kTile - 1) / mj::kTile;
        // rows of a row-major array are the image's rows, rows of an x-major array its columns
        o.op = (bits & 4) | (xmajor ? fx | fy << 1 : fy | fx << 1);
        prefix[(size_t)i + 1] = prefix[(size_t)i] + (int64_t)o.tiles_l * ((o.rows + mj::kTile - 1) / mj::kTile);
    }
    if (prefix[(size_t)n] > mj::kResizeGridX * (int64_t)65535)
        return fail(ctx, MJ_ERR_UNSUPPORTED, "%s: %lld tiles are more than one launch takes; split the batch", fn, (long long)prefix[(size_t)n]);
    int rc;
    if ((rc = upload(p, &p->d_or_images, oi.data(), oi.size())) != MJ_OK) return rc;
    if ((rc = upload(p, &p->d_or_prefix, prefix.data(), prefix.size())) != MJ_OK) return rc;
    // the stored-order pixels: a plan-owned buffer from the context's cache (64 bytes of slack: a tile row's last 16-byte load
    // may end behind the bytes it uses)
    p->src_bytes = p->info.rgb_bytes;
    MJ_HIP(ctx, alloc(p, &p->d_src, (size_t)p->src_bytes + 64));
    mj::OrientArgs &a = p->oa;
    a = mj::OrientArgs{};
    a.src = p->d_src; a.images = p->d_or_images; a.tile_prefix = p->d_or_prefix; a.total_tiles = prefix[(size_t)n];
    a.n_images = n; a.planar = p->layout >= MJ_LAYOUT_PLANAR_XMAJOR ? 1 : 0;
    if (mode) {       // (the output: the same pixels in the mode's components)
        p->out_ncomp = CO;
        p->info.rgb_bytes = p->src_bytes / C * CO;
    }
    p->resized = true;
    p->orient_only = true;
    guard.p = nullptr;
    *out = p;
    return MJ_OK;
}

}  // namespace mj

extern "C" {

int mj_host_convert_mode(int32_t mode, const uint8_t *src, int32_t src_ncomp, int64_t n_pixels, uint8_t *out) {
    if ((mode != MJ_MODE_NATIVE && mode != MJ_MODE_L && mode != MJ_MODE_RGB) || (src_ncomp != 1 && src_ncomp != 3) || n_pixels < 0 || (n_pixels && (!src || !out)))
        return MJ_ERR_INVALID;
    if (mode == MJ_MODE_NATIVE || mode == src_ncomp) memcpy(out, src, (size_t)(n_pixels * src_ncomp));
    else if (mode == MJ_MODE_L) for (int64_t i = 0; i < n_pixels; ++i) out[i] = (uint8_t)mj::mode_luma(src[3 * i], src[3 * i + 1], src[3 * i + 2]);
    else for (int64_t i = 0; i < n_pixels; ++i) out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = src[i];
    return MJ_OK;
}

}  // extern "C"
