// Mix (mj_mix; tools/mix_model.py): MixUp and CutMix over the finished outputs of a CALL — output k blended with, or patched from,
// output `partner`, which another plan may have written on another stream; so this launch belongs to no plan.  It reads one
// array of slots and writes another, every output from the array as it stood before any mixing.  The kernel, its launch, the
// call, its timing twin and the host twin.  The arithmetic and the box test are mix_rule.h's, one set of functions for both sides.
#include <math.h>

#include "plan.h"
#include "mix_rule.h"

namespace mj {

typedef unsigned int mj_mu32x4 __attribute__((ext_vector_type(4)));
template <int ES> struct MixElem;
template <> struct MixElem<1> { typedef uint8_t T; };
template <> struct MixElem<2> { typedef uint16_t T; };
template <> struct MixElem<4> { typedef uint32_t T; };

// MIXUP over this lane's vectors of one piece, the element type a template argument: the conversions are straight-line code
template <int ES, int DT>
__device__ __forceinline__ void mixup_vectors(const mj_mu32x4 (&sv)[kMixUnroll], const mj_mu32x4 (&pv)[kMixUnroll], const bool (&on)[kMixUnroll],
                                              mj_mu32x4 *const (&to)[kMixUnroll], float ws, float wp) {
    constexpr int V = 16 / ES, PER = 4 / ES;
    constexpr uint32_t EMASK = ES == 4 ? 0xFFFFFFFFu : (1u << (8 * (ES & 3))) - 1u;
#pragma unroll
    for (int u = 0; u < kMixUnroll; ++u) {
        if (!on[u]) continue;
        const uint32_t s[4] = {sv[u].x, sv[u].y, sv[u].z, sv[u].w}, p[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w};
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int q = i / PER, sh = 8 * ES * (i % PER);
            w[q] |= (mix_rule<DT>((s[q] >> sh) & EMASK, (p[q] >> sh) & EMASK, ws, wp) & EMASK) << sh;
        }
        mj_mu32x4 o;
        o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
        *to[u] = o;
    }
}

// A streaming kernel: a slot is dealt out in pieces of kMixChunkVecs 16-byte vectors, one workgroup per piece (launch_mix).  The vectors are those of the DESTINATION slot's aligned body; the output's own source
// slot is read with aligned 16-byte loads too where `src + slot` and `dst + slot` are congruent mod 16 (else, and for arrays not
// aligned to their elements, the whole slot goes element by element).  The elements in front of the first boundary and behind
// the last one go one lane each, in the slot's first piece.  The PARTNER's slot starts wherever partner * slot lands: its sixteen
// bytes are loaded from an address only known to be element-aligned, which the compiler turns into one global_load_dwordx4 (the
// target's global loads take any alignment; an aligned pair and a byte shuffle would read up to 15 bytes outside the array).
// One instance per element size serves the three kinds: the kind is uniform per workgroup, and the instance's registers are
// MIXUP's — 2 x 4 vectors and the conversions' temporaries: 85 / 76 VGPRs for 2 / 4 bytes, where the 1-byte instance, which has
// no MIXUP, takes 71 for the copies and the box test — so a MIXUP output pays nothing for the box logic and no second instance
// is made.
template <int ES>
__global__ __launch_bounds__(256) void k_mix(MixArgs a) {
    typedef typename MixElem<ES>::T T;
    constexpr int V = 16 / ES, PER = 4 / ES;            // elements per vector, per 32-bit word
    constexpr uint32_t EMASK = ES == 4 ? 0xFFFFFFFFu : (1u << (8 * (ES & 3))) - 1u;
    const int64_t n = mix_slot_elems(a.canvas);
    const int64_t items = (int64_t)a.n_outputs * a.chunks;
    const int tid = threadIdx.x;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int k = (int)(item / a.chunks), j = (int)(item - (int64_t)k * a.chunks);
        const DevMixOp op = a.ops[k];
        const T *self = static_cast<const T *>(a.src) + (int64_t)k * n;
        const T *part = static_cast<const T *>(a.src) + (int64_t)op.partner * n;
        T *out = static_cast<T *>(a.dst) + (int64_t)k * n;
        const MixBox box = mix_box(a.canvas, op.x, op.y, op.w, op.h);
        const int dtype = a.dtype;

        auto one = [&](int64_t e) {                     // a lone element
            const T s = self[e];
            if (op.kind == kMixCutmix) {
                uint32_t line, off;
                mix_locate(box, e, &line, &off);
                out[e] = mix_inside(box, line, off) ? part[e] : s;
            } else if (ES > 1 && op.kind == kMixMixup) {
                out[e] = (T)mix_rule(s, part[e], op.ws, op.wp, dtype);
            } else {
                out[e] = s;
            }
        };

        const uintptr_t sa = reinterpret_cast<uintptr_t>(self), da = reinterpret_cast<uintptr_t>(out);
        if (sa % ES || da % ES || ((sa ^ da) & 15)) {   // (no vector body: this piece's share of the elements, one by one)
            const int64_t e1 = (int64_t)(j + 1) * kMixChunkVecs * V < n ? (int64_t)(j + 1) * kMixChunkVecs * V : n;
            for (int64_t e = (int64_t)j * kMixChunkVecs * V + tid; e < e1; e += 256) one(e);
            continue;
        }
        int64_t head = (int64_t)(((16 - (da & 15)) & 15) / ES);
        if (head > n) head = n;
        const int64_t nb = (n - head) / V, tail0 = head + nb * V;
        if (j == 0) {
            if (tid < head) one(tid);
            if (tid >= 64 && tail0 + (tid - 64) < n) one(tail0 + (tid - 64));      // (fewer than V elements: V <= 16)
        }
        const int64_t v0 = (int64_t)j * kMixChunkVecs + tid;
        mj_mu32x4 sv[kMixUnroll], pv[kMixUnroll];
#pragma unroll
        for (int u = 0; u < kMixUnroll; ++u)
            if (v0 + u * 256 < nb) sv[u] = *reinterpret_cast<const mj_mu32x4 *>(self + head + (v0 + u * 256) * V);
        if (op.kind == kMixNone) {
#pragma unroll
            for (int u = 0; u < kMixUnroll; ++u)
                if (v0 + u * 256 < nb) *reinterpret_cast<mj_mu32x4 *>(out + head + (v0 + u * 256) * V) = sv[u];
        } else if (op.kind == kMixMixup) {
            if constexpr (ES > 1) {
                bool on[kMixUnroll];
                mj_mu32x4 *to[kMixUnroll];
#pragma unroll
                for (int u = 0; u < kMixUnroll; ++u) {
                    on[u] = v0 + u * 256 < nb;
                    to[u] = reinterpret_cast<mj_mu32x4 *>(out + head + (v0 + u * 256) * V);
                    if (on[u]) __builtin_memcpy(&pv[u], part + head + (v0 + u * 256) * V, 16);
                }
                if (ES == 4) mixup_vectors<ES, kDtypeF32>(sv, pv, on, to, op.ws, op.wp);
                else if (dtype == kDtypeF16) mixup_vectors<ES, kDtypeF16>(sv, pv, on, to, op.ws, op.wp);
                else mixup_vectors<ES, kDtypeBF16>(sv, pv, on, to, op.ws, op.wp);
            }
        } else {
#pragma unroll
            for (int u = 0; u < kMixUnroll; ++u) {
                if (!(v0 + u * 256 < nb)) continue;
                const int64_t e0 = head + (v0 + u * 256) * V;
                // which line the vector starts in — the one division — and, element by element, whether the box holds it
                uint32_t line, off, mask = 0;
                mix_locate(box, e0, &line, &off);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    mask |= (uint32_t)mix_inside(box, line, off) << i;
                    if (++off == box.len) { off = 0; if (++line == box.lines) line = 0; }     // (a vector may straddle lines)
                }
                mj_mu32x4 o = sv[u];
                if (mask) {                             // (a vector the box does not reach reads nothing of the partner)
                    __builtin_memcpy(&pv[u], part + e0, 16);
                    const uint32_t s[4] = {sv[u].x, sv[u].y, sv[u].z, sv[u].w}, p[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w};
                    uint32_t w[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        uint32_t m = 0;
#pragma unroll
                        for (int t = 0; t < PER; ++t) m |= ((mask >> (q * PER + t)) & 1u) ? EMASK << (8 * ES * t) : 0u;
                        w[q] = (s[q] & ~m) | (p[q] & m);
                    }
                    o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
                }
                *reinterpret_cast<mj_mu32x4 *>(out + e0) = o;
            }
        }
    }
}

hipError_t launch_mix(hipStream_t stream, MixArgs a, int esize) {
    const int64_t n = mix_slot_elems(a.canvas), V = 16 / esize;
    const int64_t chunks = ((n + V - 1) / V + kMixChunkVecs - 1) / kMixChunkVecs;
    a.chunks = (int32_t)(chunks < 1 ? 1 : chunks);
    const int64_t items = (int64_t)a.n_outputs * a.chunks;
    // One workgroup per piece (16 KiB of destination), the kernel's stride loop only for what a grid cannot hold.  The choice is
    // not measured against a capped grid that strides; what is measured is the launch beside k_copy16 over the same bytes
    // (tools/mix_probe.py, profiles/r27_mix_probe.txt).
    constexpr int64_t cap = (int64_t)1 << 22;
    const dim3 grid((unsigned)(items < cap ? items : cap)), block(256);
    if (esize == 1) hipLaunchKernelGGL(k_mix<1>, grid, block, 0, stream, a);
    else if (esize == 2) hipLaunchKernelGGL(k_mix<2>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(k_mix<4>, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace mj

namespace {

// the description of the arrays checked; false: `why` says what is wrong with it
bool check_arrays(const void *src, const void *dst, int layout, int dtype, int ncomp, int width, int height, int n_outputs, const mj_mix_op *ops,
                  char *why, size_t cap) {
    if (!src || !dst || !ops) { snprintf(why, cap, "NULL argument"); return false; }
    if (layout < 0 || layout > 3 || !mj::erase_esize(dtype) || (ncomp != 1 && ncomp != 3) || width < 1 || height < 1 || width > 65535 ||
        height > 65535 || n_outputs < 1) {
        snprintf(why, cap, "layout %d, dtype %d, %d components, %d x %d, %d outputs", layout, dtype, ncomp, width, height, n_outputs);
        return false;
    }
    const uint64_t slot = (uint64_t)width * height * ncomp * mj::erase_esize(dtype);       // (below 2^36)
    if ((uint64_t)n_outputs > ((uint64_t)1 << 62) / slot) { snprintf(why, cap, "%d outputs of %llu bytes: more than an address holds", n_outputs, (unsigned long long)slot); return false; }
    const uint64_t bytes = (uint64_t)n_outputs * slot;
    const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    if (s < d + bytes && d < s + bytes) { snprintf(why, cap, "src and dst overlap (%llu bytes each)", (unsigned long long)bytes); return false; }
    return true;
}

// the records checked against the arrays and resolved (the message names the output)
bool resolve_ops(const mj_mix_op *ops, int n_outputs, const mj::EraseCanvas &cv, int dtype, std::vector<mj::DevMixOp> &dev, char *why, size_t cap) {
    dev.assign((size_t)n_outputs, mj::DevMixOp{});
    for (int k = 0; k < n_outputs; ++k) {
        const mj_mix_op &r = ops[k];
        auto no = [&](const char *what) { snprintf(why, cap, "output %d (kind %d, partner %d): %s", k, r.kind, r.partner, what); return false; };
        mj::DevMixOp d{};
        d.kind = r.kind;
        d.partner = k;
        if (r.kind == MJ_MIX_NONE) { dev[(size_t)k] = d; continue; }
        if (r.kind != MJ_MIX_MIXUP && r.kind != MJ_MIX_CUTMIX) return no("a kind that is none of MJ_MIX_NONE, MJ_MIX_MIXUP, MJ_MIX_CUTMIX");
        if (r.partner < 0 || r.partner >= n_outputs) return no("no such partner");
        d.partner = r.partner;
        if (r.kind == MJ_MIX_MIXUP) {
            if (dtype == MJ_DTYPE_U8) return no("mixup on a uint8 output");
            if (!isfinite(r.lam) || r.lam < 0.0 || r.lam > 1.0) return no("lam is not a finite number in 0..1");
            d.ws = (float)r.lam;
            d.wp = (float)(1.0 - r.lam);
        } else {
            if (r.width < 1 || r.height < 1) {
                snprintf(why, cap, "output %d (cutmix, partner %d, x %d, y %d, %d x %d): a width or height below 1", k, r.partner, r.x, r.y, r.width, r.height);
                return false;
            }
            if (r.x < 0 || r.y < 0 || (int64_t)r.x + r.width > cv.ow || (int64_t)r.y + r.height > cv.oh) {
                snprintf(why, cap, "output %d (cutmix, partner %d, x %d, y %d, %d x %d): not inside the canvas", k, r.partner, r.x, r.y, r.width, r.height);
                return false;
            }
            d.x = r.x; d.y = r.y; d.w = r.width; d.h = r.height;
        }
        dev[(size_t)k] = d;
    }
    return true;
}

template <typename T>
void host_mix(const T *src, T *dst, const mj::EraseCanvas &cv, int dtype, const std::vector<mj::DevMixOp> &ops) {
    const int64_t n = mj::mix_slot_elems(cv);
    for (size_t k = 0; k < ops.size(); ++k) {
        const mj::DevMixOp &op = ops[k];
        const T *self = src + (int64_t)k * n, *part = src + (int64_t)op.partner * n;
        T *out = dst + (int64_t)k * n;
        const mj::MixBox box = mj::mix_box(cv, op.x, op.y, op.w, op.h);
        for (int64_t e = 0; e < n; ++e) {
            if (op.kind == mj::kMixCutmix) {
                uint32_t line, off;
                mj::mix_locate(box, e, &line, &off);
                out[e] = mj::mix_inside(box, line, off) ? part[e] : self[e];
            } else if (op.kind == mj::kMixMixup) {
                out[e] = (T)mj::mix_rule(self[e], part[e], op.ws, op.wp, dtype);
            } else {
                out[e] = self[e];
            }
        }
    }
}

// the records into the context's device buffer, behind the previous mix launch (which reads it), ahead of this one on `s`
int stage_ops(mj_context *ctx, hipStream_t s, const std::vector<mj::DevMixOp> &dev) {
    const size_t bytes = dev.size() * sizeof(mj::DevMixOp);
    if (ctx->mix_flying) { MJ_HIP(ctx, hipEventSynchronize(ctx->mix_done)); ctx->mix_flying = false; }
    if (!ctx->mix_done) MJ_HIP(ctx, hipEventCreateWithFlags(&ctx->mix_done, hipEventDisableTiming));
    if (bytes > ctx->mix_cap) {
        if (ctx->h_mix) { (void)hipHostFree(ctx->h_mix); ctx->h_mix = nullptr; }
        if (ctx->d_mix) { (void)hipFree(ctx->d_mix); ctx->d_mix = nullptr; }
        ctx->mix_cap = 0;
        const size_t cap = bytes + bytes / 2 + 4096;
        MJ_HIP(ctx, hipHostMalloc(&ctx->h_mix, cap, hipHostMallocDefault));
        MJ_HIP(ctx, hipMalloc(&ctx->d_mix, cap));
        ctx->mix_cap = cap;
    }
    memcpy(ctx->h_mix, dev.data(), bytes);
    MJ_HIP(ctx, hipMemcpyAsync(ctx->d_mix, ctx->h_mix, bytes, hipMemcpyHostToDevice, s));
    return MJ_OK;
}

int mix_prepare(mj_context *ctx, const char *fn, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t width,
                int32_t height, int32_t n_outputs, const mj_mix_op *ops, hipStream_t s, mj::MixArgs *a) {
    char why[256];
    if (!check_arrays(src, dst, layout, dtype, ncomp, width, height, n_outputs, ops, why, sizeof(why))) return fail(ctx, MJ_ERR_INVALID, "%s: %s", fn, why);
    const mj::EraseCanvas cv{width, height, ncomp, layout};
    std::vector<mj::DevMixOp> dev;
    if (!resolve_ops(ops, n_outputs, cv, dtype, dev, why, sizeof(why))) return fail(ctx, MJ_ERR_INVALID, "%s: %s", fn, why);
    MJ_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = stage_ops(ctx, s, dev)) return rc;
    a->src = src; a->dst = dst; a->ops = static_cast<const mj::DevMixOp *>(ctx->d_mix);
    a->canvas = cv; a->dtype = dtype; a->n_outputs = n_outputs; a->chunks = 0;
    return MJ_OK;
}

}  // namespace

extern "C" {

int mj_mix(mj_context *ctx, void *stream, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t width, int32_t height,
           int32_t n_outputs, const mj_mix_op *ops) {
    if (!ctx) return MJ_ERR_INVALID;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    mj::MixArgs a{};
    if (int rc = mix_prepare(ctx, "mj_mix", src, dst, layout, dtype, ncomp, width, height, n_outputs, ops, s, &a)) return rc;
    // The event goes behind the staging copy whether or not the launch went out: the next call must not rewrite the pinned block
    // under a copy that is still queued.  Where the event cannot be recorded either, the stream is drained here instead.
    const hipError_t launched = mj::launch_mix(s, a, mj::erase_esize(dtype));
    const hipError_t recorded = hipEventRecord(ctx->mix_done, s);
    if (recorded == hipSuccess) ctx->mix_flying = true;
    else (void)hipStreamSynchronize(s);
    MJ_HIP(ctx, launched);
    MJ_HIP(ctx, recorded);
    return MJ_OK;
}

int mj_mix_time(mj_context *ctx, int iters, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t width, int32_t height,
                int32_t n_outputs, const mj_mix_op *ops, float *ms_out) {
    if (!ctx || iters <= 0 || !ms_out) return MJ_ERR_INVALID;
    hipStream_t s = ctx->stream;
    mj::MixArgs a{};
    if (int rc = mix_prepare(ctx, "mj_mix_time", src, dst, layout, dtype, ncomp, width, height, n_outputs, ops, s, &a)) return rc;
    // (the staged records are read until the last launch ends: every way out of here, a failure too, leaves the stream drained, so
    // mix_flying stays false)
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{s};
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    MJ_HIP(ctx, hipEventCreate(&ev.a));
    MJ_HIP(ctx, hipEventCreate(&ev.b));
    MJ_HIP(ctx, mj::launch_mix(s, a, mj::erase_esize(dtype)));         // (warm)
    MJ_HIP(ctx, hipEventRecord(ev.a, s));
    for (int i = 0; i < iters; ++i) MJ_HIP(ctx, mj::launch_mix(s, a, mj::erase_esize(dtype)));
    MJ_HIP(ctx, hipEventRecord(ev.b, s));
    MJ_HIP(ctx, hipEventSynchronize(ev.b));
    float ms = 0.f;
    MJ_HIP(ctx, hipEventElapsedTime(&ms, ev.a, ev.b));
    *ms_out = ms / iters;
    return MJ_OK;
}

int mj_host_mix(const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t width, int32_t height, int32_t n_outputs,
                const mj_mix_op *ops) {
    const char *fn = "mj_host_mix";
    char why[256];
    if (!check_arrays(src, dst, layout, dtype, ncomp, width, height, n_outputs, ops, why, sizeof(why))) return fail(nullptr, MJ_ERR_INVALID, "%s: %s", fn, why);
    const mj::EraseCanvas cv{width, height, ncomp, layout};
    std::vector<mj::DevMixOp> dev;
    if (!resolve_ops(ops, n_outputs, cv, dtype, dev, why, sizeof(why))) return fail(nullptr, MJ_ERR_INVALID, "%s: %s", fn, why);
    switch (mj::erase_esize(dtype)) {
        case 1: host_mix(static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst), cv, dtype, dev); break;
        case 2: host_mix(static_cast<const uint16_t *>(src), static_cast<uint16_t *>(dst), cv, dtype, dev); break;
        default: host_mix(static_cast<const uint32_t *>(src), static_cast<uint32_t *>(dst), cv, dtype, dev); break;
    }
    return MJ_OK;
}

}  // extern "C"
