// mj_plan_create_with: check and normalise the request, validate the batch description, choose the forms its stages take (form_select.h), build the tables and
// descriptors and upload them.  Host-side only.
#include <math.h>

#include "plan.h"

namespace {

// zig-zag index -> natural index v*8+u (row = vertical frequency); blocks and quantisation tables live on the
// device in this order (see huffman.hip / reconstruct_fast.hip)
const uint8_t kNatOfZz[64] = {
    0,  1,  8, 16,  9,  2,  3, 10, 17, 24, 32, 25, 18, 11,  4,  5,
   12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,  6,  7, 14, 21, 28,
   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
   58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

bool sampling_class(const mj_image_desc &d, int &hmax, int &vmax) {
    if (d.ncomp == 1) { hmax = vmax = 1; return true; }
    if (d.ncomp != 3) return false;
    if (d.hs[1] != 1 || d.vs[1] != 1 || d.hs[2] != 1 || d.vs[2] != 1) return false;
    hmax = d.hs[0]; vmax = d.vs[0];
    return ((hmax == 1 || hmax == 2) && (vmax == 1 || vmax == 2)) || (hmax == 4 && vmax == 1);
}

// Any other three-component layout with factors 1..4 (4:1:0, 1x4, factors of 3, chroma above 1x1, luma below the chroma
// resolution ...): decoded by the wave form of stage 1 and k_reconstruct_generic.  The reference takes them all (:205-240).
bool generic_sampling(const mj_image_desc &d, int &hmax, int &vmax) {
    if (d.ncomp != 3) return false;
    hmax = vmax = 1;
    int blocks = 0;
    for (int c = 0; c < 3; ++c) {
        if (d.hs[c] < 1 || d.hs[c] > 4 || d.vs[c] < 1 || d.vs[c] > 4) return false;
        hmax = std::max(hmax, (int)d.hs[c]); vmax = std::max(vmax, (int)d.vs[c]);
        blocks += d.hs[c] * d.vs[c];
    }
    return blocks <= mj::kMaxBlocksPerMcu;
}

// every code of at most `width` bits of a table, in canonical order (jpeg_decoder.py:366-377): fn(code, length, symbol)
template <class F>
void for_each_short_code(const mj_huff_spec &h, int width, F &&fn) {
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        code <<= 1;
        for (int i = 0; i < h.bits[l - 1] && k < 256; ++i, ++k, ++code)
            if (l <= width && code < (1 << l)) fn(code, l, (int)h.vals[k]);
    }
}
// ... and the entries of a `width`-bit LUT that start with that code := entry, where no shorter code has them
void fill_lut(uint16_t *lut, int width, int code, int l, uint16_t entry) {
    for (int f = 0, shift = width - l; f < (1 << shift); ++f)
        if (uint16_t &e = lut[(code << shift) | f]; e == 0) e = entry;
}

// describe_images: the batch's restart segments and running totals (host side; the plan gets what it keeps)
struct BatchSegments {
    std::vector<mj::DevSegment> segs;      // what stages 0 and 1 read
    std::vector<mj::DevSegment> full_segs; // GPU-segmented window plans that need only some: every segment the marker scan fills
    std::vector<int32_t> gather;           // ... and which of them the windows need
    std::vector<mj::DevScanJob> jobs;      // MJ_FLAG_GPU_SEGMENT: one marker-scan job per image
    std::vector<int64_t> mcu_prefix, win_prefix;       // first MCU / first window MCU of every image (+ total)
    int64_t blk = 0, mcu = 0, rgb = 0, pix = 0, ent = 0;
};
// lane_tables: how each table is used — bit 0 = as a DC table, bit 1 = as an AC table (the two LUT formats differ)
struct TableRoles { std::vector<int> role; bool both_roles = false, dc_fits = true; };
// choose_forms: what the later steps need of the choice — the byte lengths of S.segs, the per-workgroup table lists (many_tabs)
struct Forms { bool many_tabs = false, want_sync = false; std::vector<int32_t> seg_len, wl_lanes, wl_count; };

int check_batch(mj_context *ctx, const mj_batch *b, bool roi_plan, mj_plan **out) {
    if (!ctx) return MJ_ERR_INVALID;
    if (!b || !out) return fail(ctx, MJ_ERR_INVALID, "mj_plan_create: NULL argument");
    *out = nullptr;
    if (b->n_images <= 0 || !b->images) return fail(ctx, MJ_ERR_INVALID, "mj_plan_create: empty batch");
    if (b->layout < MJ_LAYOUT_XMAJOR || b->layout > MJ_LAYOUT_PLANAR_ROWMAJOR)
        return fail(ctx, MJ_ERR_INVALID, "mj_plan_create: unknown layout %d", b->layout);
    if (b->n_qt <= 0 || !b->qt) return fail(ctx, MJ_ERR_INVALID, "mj_plan_create: no quantisation tables");
    if (roi_plan && (b->flags & (MJ_FLAG_KEEP_COEF | MJ_FLAG_KEEP_PLANES | MJ_FLAG_KEEP_IDCT)))
        return fail(ctx, MJ_ERR_INVALID, "%s: the seam outputs (MJ_FLAG_KEEP_*) are whole-image; a window plan has none", mj::kCreateFn);
    MJ_HIP(ctx, hipSetDevice(ctx->device));
    return MJ_OK;
}

// The steps of plan creation and what each of them is given (roi_plan: a window plan; rois == NULL: every window is the whole image).
// They run in mj::plan_create_common's order, which is also the order of the plan's requests to the context's buffer cache: which
// cached block a plan gets depends on it (tests/test_plan_shapes.py holds it).
struct Create {
    mj_context *ctx; const mj_batch *b; mj_plan *p; const mj_roi *rois; bool roi_plan, have_entropy, prog;

    // image i's descriptor (and window), checked
    int image_descriptor(int i, BatchSegments &S, bool &common) {
        const mj_image_desc &d = b->images[i];
        mj::DevImage &im = p->h_images[i];
        memset(&im, 0, sizeof(im));
        int hmax, vmax;
        if (d.width <= 0 || d.height <= 0 || d.width > 65535 || d.height > 65535)
            return fail(ctx, MJ_ERR_INVALID, "image %d: bad dimensions %dx%d", i, d.width, d.height);
        common = sampling_class(d, hmax, vmax);
        if (!common && !generic_sampling(d, hmax, vmax))
            return fail(ctx, MJ_ERR_UNSUPPORTED,
                        "image %d: sampling layout not supported by the MI355X path (ncomp=%d, Y %dx%d, Cb %dx%d, Cr %dx%d); "
                        "supported: one component, or three with factors 1..4 and at most %d blocks per MCU", i, d.ncomp, d.hs[0], d.vs[0],
                        d.hs[1], d.vs[1], d.hs[2], d.vs[2], mj::kMaxBlocksPerMcu);
        if (!common && prog) {
            // the reference's final pass (:1319-1362) resizes every 8x8 block of a component to the full MCU shape and stores it
            // into ratio x ratio blocks: that only fits when the component is 1x1 — or is not resized at all
            for (int c = 0; c < 3; ++c)
                if (!((d.hs[c] == 1 && d.vs[c] == 1) || (d.hs[c] == hmax && d.vs[c] == vmax)))
                    return fail(ctx, MJ_ERR_UNSUPPORTED, "image %d: scan-by-scan files need every component at 1x1 or at the full resolution "
                                "(the reference's final pass cannot place the blocks of a %dx%d component under %dx%d: ValueError)", i,
                                d.hs[c], d.vs[c], hmax, vmax);
        }
        if (i == 0) { p->hmax = hmax; p->vmax = vmax; p->ncomp = d.ncomp; }
        else if (hmax != p->hmax || vmax != p->vmax || d.ncomp != p->ncomp || common == p->generic ||
                 (p->generic && (memcmp(d.hs, b->images[0].hs, sizeof(d.hs)) || memcmp(d.vs, b->images[0].vs, sizeof(d.vs)))))
            return fail(ctx, MJ_ERR_UNSUPPORTED, "image %d: a plan holds one sampling layout; split the batch by layout", i);
        const int mw = d.ncomp == 1 ? 8 : 8 * hmax, mh = d.ncomp == 1 ? 8 : 8 * vmax;
        if (d.mcu_count_h != (d.width + mw - 1) / mw || d.mcu_count_v != (d.height + mh - 1) / mh)
            return fail(ctx, MJ_ERR_INVALID, "image %d: MCU counts %dx%d do not match %dx%d with %dx%d MCUs", i,
                        d.mcu_count_h, d.mcu_count_v, d.width, d.height, mw, mh);
        if (roi_plan) {
            mj::DevWindow &w = p->h_win[i];
            if (rois) { w.x0 = rois[i].x; w.y0 = rois[i].y; w.w = rois[i].width; w.h = rois[i].height; }
            else { w.x0 = 0; w.y0 = 0; w.w = d.width; w.h = d.height; }
            if (w.w <= 0 || w.h <= 0 || w.x0 < 0 || w.y0 < 0 || (int64_t)w.x0 + w.w > d.width || (int64_t)w.y0 + w.h > d.height)
                return fail(ctx, MJ_ERR_INVALID, "image %d: window (x %d, y %d, width %d, height %d) is empty or not inside the %dx%d image",
                            i, w.x0, w.y0, w.w, w.h, d.width, d.height);
            w.mx0 = w.x0 / mw; w.my0 = w.y0 / mh;
            w.mcw = (w.x0 + w.w - 1) / mw - w.mx0 + 1; w.mch = (w.y0 + w.h - 1) / mh - w.my0 + 1;
            S.win_prefix[i + 1] = S.win_prefix[i] + (int64_t)w.mcw * w.mch;
        }
        im.width = d.width; im.height = d.height; im.ncomp = d.ncomp;
        p->max_pixels = std::max(p->max_pixels, (int64_t)d.width * d.height);
        im.hmax = hmax; im.vmax = vmax;
        im.blocks_per_mcu = d.ncomp == 1 ? 1 : hmax * vmax + 2;
        im.generic = common ? 0 : 1;
        if (!common) im.blocks_per_mcu = d.hs[0] * d.vs[0] + d.hs[1] * d.vs[1] + d.hs[2] * d.vs[2];
        im.mcu_count_h = d.mcu_count_h; im.mcu_count_v = d.mcu_count_v;
        im.restart_interval = d.restart_interval;
        // per-block component / table slots, decode order (jpeg_decoder.py:774, :805)
        int nb = 0;
        for (int c = 0; c < d.ncomp; ++c) {
            if (d.qt_sel[c] < 0 || d.qt_sel[c] >= b->n_qt) return fail(ctx, MJ_ERR_INVALID, "image %d: qt_sel out of range", i);
            im.qt_index[c] = d.qt_sel[c];
            int dslot = 0, aslot = 0;
            if (have_entropy && !prog) {
                if (d.dc_sel[c] < 0 || d.dc_sel[c] >= b->n_huff || d.ac_sel[c] < 0 || d.ac_sel[c] >= b->n_huff)
                    return fail(ctx, MJ_ERR_INVALID, "image %d: Huffman table selector out of range", i);
                auto slot_of = [&](int t) {
                    for (int s = 0; s < im.n_tabs; ++s) if (im.tab_index[s] == t) return s;
                    im.tab_index[im.n_tabs] = t;
                    return im.n_tabs++;
                };
                dslot = slot_of(d.dc_sel[c]);
                aslot = slot_of(d.ac_sel[c]);
            }
            const int rep = d.ncomp == 1 ? 1 : (common ? (c == 0 ? hmax * vmax : 1) : d.hs[c] * d.vs[c]);
            im.comp_h[c] = (uint8_t)(d.ncomp == 1 ? 1 : (common ? (c == 0 ? hmax : 1) : d.hs[c]));
            im.comp_v[c] = (uint8_t)(d.ncomp == 1 ? 1 : (common ? (c == 0 ? vmax : 1) : d.vs[c]));
            im.comp_first[c] = (uint8_t)nb;
            for (int r = 0; r < rep; ++r, ++nb) {
                im.blk_comp[nb] = (uint8_t)c; im.blk_dc_slot[nb] = (uint8_t)dslot; im.blk_ac_slot[nb] = (uint8_t)aslot;
            }
        }
        if (im.n_tabs > p->lut_slots) p->lut_slots = im.n_tabs;
        im.block_off = S.blk; im.mcu_off = S.mcu; im.rgb_off = S.rgb; im.pix_off = S.pix;
        if (i > 0 && (d.width != b->images[0].width || d.height != b->images[0].height)) p->uniform = false;
        return MJ_OK;
    }

    // image i's restart segments (and marker-scan job), checked; a window plan keeps the ones its window needs
    int image_segments(int i, BatchSegments &S) {
        const mj_image_desc &d = b->images[i];
        const int64_t mcus = (int64_t)d.mcu_count_h * d.mcu_count_v;
        const int64_t want = d.restart_interval > 0 ? (mcus + d.restart_interval - 1) / d.restart_interval : 1;
        const bool gpu_seg = (b->flags & MJ_FLAG_GPU_SEGMENT) != 0;
        if (d.n_segments != (gpu_seg ? 1 : want))
            return fail(ctx, MJ_ERR_INVALID, "image %d: %d restart segments given, %lld expected (restart interval %d, %lld MCUs)",
                        i, d.n_segments, (long long)(gpu_seg ? 1 : want), d.restart_interval, (long long)mcus);
        if (d.first_segment < 0 || d.first_segment + d.n_segments > b->n_segments)
            return fail(ctx, MJ_ERR_INVALID, "image %d: segment range outside seg_begin/seg_end", i);
        if (gpu_seg) {      // one byte range per image; stage 0 finds the markers and fills begin/len (destuff.hip)
            const int64_t sb = b->seg_begin[d.first_segment], se = b->seg_end[d.first_segment];
            if (sb < 0 || se < sb || se > b->blob_len || se - sb > 0x7fff0000)
                return fail(ctx, MJ_ERR_INVALID, "image %d: bad byte range [%lld, %lld)", i, (long long)sb, (long long)se);
            mj::DevScanJob jb{};
            jb.begin = sb; jb.end = se; jb.first_seg = (int64_t)S.segs.size(); jb.n_seg = (int32_t)want; jb.image = i;
            S.jobs.push_back(jb);
            S.ent += se - sb;
        }
        for (int s = 0; s < (int)want; ++s) {
            mj::DevSegment g{};
            g.image = i;
            g.mcu0 = d.restart_interval > 0 ? s * d.restart_interval : 0;
            g.n_mcu = (int32_t)(d.restart_interval > 0 ? std::min<int64_t>(d.restart_interval, mcus - g.mcu0) : mcus);
            g.last = s == (int)want - 1;
            // a window plan decodes a restart segment only where one of its MCUs (raster order; a segment may span rows) lies in
            // the window's MCU rectangle
            bool need = true;
            if (roi_plan) {
                const mj::DevWindow &w = p->h_win[i];
                const int64_t m0 = g.mcu0, m1 = m0 + g.n_mcu, mch_ = d.mcu_count_h;
                need = false;
                for (int64_t r = std::max<int64_t>(m0 / mch_, w.my0); r <= std::min<int64_t>((m1 - 1) / mch_, w.my0 + w.mch - 1) && !need; ++r) {
                    const int64_t c0 = std::max<int64_t>(m0, r * mch_) - r * mch_, c1 = std::min<int64_t>(m1, (r + 1) * mch_) - r * mch_;
                    need = c0 < w.mx0 + w.mcw && c1 > w.mx0;
                }
            }
            if (gpu_seg) {
                g.begin = b->seg_begin[d.first_segment]; g.len = 0;
                if (roi_plan && need) S.gather.push_back((int32_t)S.segs.size());
            } else {
                const int64_t sb = b->seg_begin[d.first_segment + s], se = b->seg_end[d.first_segment + s];
                if (sb < 0 || se < sb || se > b->blob_len || se - sb > 0x7fff0000)
                    return fail(ctx, MJ_ERR_INVALID, "image %d segment %d: bad byte range [%lld, %lld)", i, s, (long long)sb, (long long)se);
                g.begin = sb; g.len = (int32_t)(se - sb);
                if (!need) continue;
                S.ent += se - sb;
            }
            S.segs.push_back(g);
        }
        return MJ_OK;
    }

    // the images' descriptors, windows, restart segments and marker-scan jobs, and the batch's totals
    int describe_images(BatchSegments &S) {
        S.mcu_prefix.assign(b->n_images + 1, 0);
        p->h_images.resize(b->n_images);
        if (roi_plan) { p->h_win.resize(b->n_images); S.win_prefix.assign(b->n_images + 1, 0); }
        p->uniform = true;
        p->lut_slots = 1;
        for (int i = 0; i < b->n_images; ++i) {
            const mj_image_desc &d = b->images[i];
            bool common;
            if (int rc = image_descriptor(i, S, common)) return rc;
            S.mcu_prefix[i] = S.mcu;
            if (have_entropy && !prog)
                if (int rc = image_segments(i, S)) return rc;
            const int64_t mcus = (int64_t)d.mcu_count_h * d.mcu_count_v;
            S.blk += mcus * p->h_images[i].blocks_per_mcu;
            S.mcu += mcus;
            const int64_t opix = roi_plan ? (int64_t)p->h_win[i].w * p->h_win[i].h : (int64_t)d.width * d.height;     // (window plans: the window's)
            S.rgb += opix * d.ncomp;
            S.pix += opix;
        }
        S.mcu_prefix[b->n_images] = S.mcu;
        // MJ_FLAG_GPU_SEGMENT window plans: stages 0 and 1 get the needed segments only (gathered behind the marker scan, which fills
        // the whole list); where every segment is needed there is nothing to gather
        if (roi_plan && !S.jobs.empty() && S.gather.size() < S.segs.size()) {
            S.full_segs.swap(S.segs);
            for (int32_t k : S.gather) S.segs.push_back(S.full_segs[(size_t)k]);
        }
        return MJ_OK;
    }

    // the totals into the plan; the image descriptors, the MCU prefix and the quantisation tables onto the device
    int upload_descriptors(const BatchSegments &S) {
        p->mcus_per_image = (int32_t)(S.mcu / b->n_images);
        p->info.total_blocks = S.blk; p->info.total_mcus = S.mcu; p->info.total_pixels = S.pix;
        p->info.rgb_bytes = S.rgb; p->info.entropy_bytes = S.ent;
        p->n_segs = (int64_t)S.segs.size();
        if (int rc = upload(p, &p->d_images, p->h_images.data(), p->h_images.size())) return rc;
        if (int rc = upload(p, &p->d_mcu_prefix, S.mcu_prefix.data(), S.mcu_prefix.size())) return rc;
        std::vector<uint16_t> qn((size_t)b->n_qt * 64);
        for (int t = 0; t < b->n_qt; ++t)
            for (int z = 0; z < 64; ++z) {
                const int n = kNatOfZz[z];
                qn[(size_t)t * 64 + (p->transposed ? ((n & 7) << 3 | n >> 3) : n)] = b->qt[(size_t)t * 64 + z];
            }
        return upload(p, &p->d_qt, qn.data(), qn.size());
    }

    // The fast stage 2 hands its work out in JOBS (reconstruct_fast.hip): up to `chunk_strips` vertically consecutive strips
    // (a strip = fast_tile_mcus() MCUs) of one MCU column — a whole column where that is at most 24 strips (1080p: 17),
    // else equal pieces of one.  Jobs are numbered image by image; the kernel's ticket counter is the (zero) word behind
    // the prefix.
    int stage2_jobs() {
        const std::vector<mj::DevImage> &imgs = p->h_images; const std::vector<mj::DevWindow> &wins = p->h_win;
        const int tm = p->generic ? 1 : mj::fast_tile_mcus(p->hmax, p->vmax, p->ncomp, p->transposed);
        // strips run down the MCU columns of the image the kernel sees (row-major plans: the transposed one; window plans: the windows' MCU rectangles)
        auto kcols = [&](int i) { return roi_plan ? (p->transposed ? wins[i].mch : wins[i].mcw) : (p->transposed ? imgs[i].mcu_count_v : imgs[i].mcu_count_h); };
        auto krows = [&](int i) { return roi_plan ? (p->transposed ? wins[i].mcw : wins[i].mch) : (p->transposed ? imgs[i].mcu_count_h : imgs[i].mcu_count_v); };
        int max_spc = 1;
        for (int i = 0; i < b->n_images; ++i) max_spc = std::max(max_spc, (krows(i) + tm - 1) / tm);
        const int pieces_max = (max_spc + 23) / 24;
        p->chunk_strips = (max_spc + pieces_max - 1) / pieces_max;
        if (const char *e = mj::opt("MJ_STAGE2_CHUNK")) { const int v = atoi(e); if (v >= 1 && v <= 4096) p->chunk_strips = v; }
        std::vector<int64_t> tp(b->n_images + 1, 0);
        for (int i = 0; i < b->n_images; ++i) {
            const int spc = (krows(i) + tm - 1) / tm;
            tp[i + 1] = tp[i] + (int64_t)kcols(i) * ((spc + p->chunk_strips - 1) / p->chunk_strips);
        }
        p->total_jobs = tp[b->n_images];
        // a ticket should be worth ~400 blocks of IDCT work (a 1080p 4:2:0 column: 17 strips x 24 blocks): consecutive jobs per ticket
        const int blocks_per_strip = p->generic ? 1 : tm * (p->ncomp == 1 ? 1 : p->hmax * p->vmax + 2);
        const int per_job = std::max(1, blocks_per_strip * std::min(p->chunk_strips, max_spc));
        p->jobs_per_ticket = std::max(1, (400 + per_job / 2) / per_job);
        p->jobs_per_image = (int32_t)(tp[1] - tp[0]);
        tp.insert(tp.end(), 5, 0);         // the ticket counter, a spare word, the three level counters of mj_plan_idct_levels
        return upload(p, &p->d_job_prefix, tp.data(), tp.size());
    }

    // The Huffman tables as the stage-1 kernels read them: code books, the lane kernel's 11-bit LUTs (AC tables: length, zero run and
    // size ready for use, end of block = a run of 64), the resolved 13-bit AC tables, the unified format of huffman_sync.hip
    int lane_tables(TableRoles &T) {
        std::vector<mj::DevHuff> hh(b->n_huff);
        for (int t = 0; t < b->n_huff; ++t) mj::build_dev_huff(b->huff[t], hh[t]);
        if (int rc = upload(p, &p->d_huff, hh.data(), hh.size())) return rc;
        p->n_huff = b->n_huff;
        T.role.assign(b->n_huff, 0);
        for (const mj::DevImage &im : p->h_images)
            for (int k2 = 0; k2 < im.blocks_per_mcu && k2 < mj::kMaxBlocksPerMcu; ++k2) {
                T.role[im.tab_index[im.blk_dc_slot[k2]]] |= 1;
                T.role[im.tab_index[im.blk_ac_slot[k2]]] |= 2;
            }
        for (int t = 0; t < b->n_huff; ++t) T.both_roles = T.both_roles || T.role[t] == 3;
        const int LB = mj::kLaneLutBits, LS = 1 << LB;
        std::vector<uint16_t> l11((size_t)b->n_huff * LS, 0), lu((size_t)b->n_huff * LS, 0);
        for (int t = 0; t < b->n_huff; ++t) {
            const bool ac = (T.role[t] & 2) != 0;
            for_each_short_code(b->huff[t], LB, [&](int code, int l, int hv) {
                const uint16_t run_size = (uint16_t)((l << 11) | ((hv == 0 ? 64 : hv >> 4) << 4) | (hv & 15));
                fill_lut(&l11[(size_t)t * LS], LB, code, l, ac ? run_size : (uint16_t)((l << 8) | hv));
                fill_lut(&lu[(size_t)t * LS], LB, code, l, ac ? run_size : (uint16_t)((l << 11) | (hv & 15)));
                if (!ac && hv > 15) T.dc_fits = false;           // a DC size above 15 has no place in the unified format
            });
        }
        if (int rc = upload(p, &p->d_lut11, l11.data(), l11.size())) return rc;
        // the fast variant of the lane form (huffman_lanes13.hip): 13-bit AC tables whose entries are finished symbols
        // — bits consumed, step of the write position, EXTENDed coefficient (jpeg_decoder.py:834-866, :1636-1646) —
        // wherever code + value bits fit the index; every table must have one role and the lot must fit LDS
        // (a fused launch keeps smaller copies in LDS beside its reconstruction wavefronts' strips: fused_setup)
        int n_ac = 0, n_dc = 0;
        uint64_t ac_pk = 0, dc_pk = 0, dct_pk = 0;
        bool ok13 = b->n_huff <= 8 && !T.both_roles && !prog;
        for (int t = 0; t < b->n_huff && ok13; ++t) {
            if (T.role[t] == 2) ac_pk |= (uint64_t)n_ac++ << (8 * t);
            else if (T.role[t] == 1) { dc_pk |= (uint64_t)n_dc << (8 * t); dct_pk |= (uint64_t)t << (8 * n_dc); ++n_dc; }
        }
        const char *f13 = mj::opt("MJ_HUFFMAN");
        if (f13 && !strcmp(f13, "lanes11")) ok13 = false;
        std::vector<uint32_t> l13;
        const int ab13[4] = {13, 13, 13, 13};
        int off13[4] = {0, 0, 0, 0}, total13 = 0;
        if (ok13 && mj::lanes13_fits(n_ac, n_dc) && mj::build_resolved_tables(b, T.role, ac_pk, n_ac, ab13, mj::kLanes13SlotBytes, l13, off13, total13)) {
            if (int rc = upload(p, &p->d_lut13, l13.data(), l13.size())) return rc;
            p->n_ac13 = n_ac; p->n_dc13 = n_dc;
            p->ac_slot_pk = ac_pk; p->dc_slot_pk = dc_pk; p->dc_tab_pk = dct_pk;
        }
        return upload(p, &p->d_lut11u, lu.data(), lu.size());
    }

    // More tables than LDS holds (every file with its own optimised tables): a workgroup loads just the tables of its units' images.
    // The lists of one launch shape, units_per_wg consecutive units per workgroup: false where a workgroup needs more than `cap` tables
    static bool wg_lists(const std::vector<mj::DevImage> &imgs, const std::vector<int32_t> &unit_image, int64_t units_per_wg, int cap, std::vector<int32_t> &lists) {
        const int64_t n_wg = ((int64_t)unit_image.size() + units_per_wg - 1) / units_per_wg;
        lists.assign((size_t)n_wg * mj::kMaxWgTables, -1);
        for (int64_t g = 0; g < n_wg; ++g) {
            int32_t *l = lists.data() + (size_t)g * mj::kMaxWgTables;
            int n = 0, last_img = -1;
            const int64_t u1 = std::min<int64_t>((g + 1) * units_per_wg, (int64_t)unit_image.size());
            for (int64_t u = g * units_per_wg; u < u1; ++u) {
                const int img = unit_image[(size_t)u];
                if (img == last_img) continue;
                last_img = img;
                for (int k2 = 0; k2 < imgs[img].n_tabs; ++k2) {
                    const int t = imgs[img].tab_index[k2];
                    bool seen = false;
                    for (int j = 0; j < n; ++j) seen = seen || l[j] == t;
                    if (seen) continue;
                    if (n == cap) return false;
                    l[n++] = t;
                }
            }
        }
        return true;
    }
    // ... with 8, or else 16, tables per workgroup (64 KiB of LUTs: two workgroups per CU, still not the wave form), for the lane launch
    // over restart segments (cb == 0) — or the counting rounds (256 chunks per workgroup) and the lane launch over chunks of cb bytes
    bool wg_table_lists(const BatchSegments &S, int cb, Forms &F) {
        std::vector<int32_t> unit_image;
        for (const auto &g : S.segs)
            for (int j = 0; j < (cb ? std::max(1, (g.len + cb - 1) / cb) : 1); ++j) unit_image.push_back(g.image);
        bool ok_count = cb == 0, ok_lanes = false;
        for (int cap = 8; cap <= mj::kMaxWgTables && !ok_count; cap *= 2) {
            ok_count = wg_lists(p->h_images, unit_image, 256, cap, F.wl_count);
            p->wg_slots_count = cap;
        }
        for (int cap = 8; cap <= mj::kMaxWgTables && !ok_lanes; cap *= 2) {
            ok_lanes = wg_lists(p->h_images, unit_image, 4 * (int64_t)mj::lanes_per_wave((int64_t)unit_image.size(), cap), cap, F.wl_lanes);
            p->wg_slots_lanes = cap;
        }
        return ok_count && ok_lanes;
    }

    // which form stage 1 takes: the rule is form_select.h's (choose_stage1_form), here are its inputs
    void choose_forms(BatchSegments &S, const TableRoles &T, Forms &F) {
        std::vector<mj::DevSegment> &segs = S.segs;
        const std::vector<mj::DevScanJob> &jobs = S.jobs;
        // stage 0 places segment i's stream at dword (begin_i >> 2) + i: that needs the segments (or, with the GPU
        // marker scan, the images' byte ranges) in ascending, non-overlapping blob order — what any packer produces
        bool ordered = true;
        for (size_t i = 1; jobs.empty() && i < segs.size() && ordered; ++i) ordered = segs[i].begin >= segs[i - 1].begin + segs[i - 1].len;
        for (size_t i = 1; i < jobs.size() && ordered; ++i) ordered = jobs[i].begin >= jobs[i - 1].end;
        F.many_tabs = b->n_huff > mj::kMaxLaneTables;
        const bool many_ok_dri = !(F.many_tabs && !prog && !T.both_roles) || wg_table_lists(S, 0, F);
        if (const char *e = mj::opt("MJ_SYNC_ROUNDS")) { const int v = atoi(e); if (v >= 0 && v <= 64) p->sync_rounds = v; }
        if (const char *e = mj::opt("MJ_SYNC_WARM")) p->sync_warm_bits = atoi(e) * 8;
        bool one_seg_each = true;
        for (const auto &jb : jobs) one_seg_each = one_seg_each && jb.n_seg == 1;
        if (!jobs.empty() && one_seg_each)
            for (size_t i = 0; i < jobs.size(); ++i) segs[(size_t)jobs[i].first_seg].len = (int32_t)(jobs[i].end - jobs[i].begin);   // upper bound; the scan writes the real one
        F.seg_len.resize(segs.size());
        for (size_t i = 0; i < segs.size(); ++i) F.seg_len[i] = segs[i].len;
        mj::FormInputs fin;
        fin.seg_len = F.seg_len.data(); fin.n_segs = (int64_t)segs.size(); fin.blob_len = (uint64_t)b->blob_len; fin.n_huff = b->n_huff;
        fin.both_roles = T.both_roles; fin.ordered = ordered; fin.progressive = prog; fin.generic = p->generic;
        fin.gpu_segment = !jobs.empty(); fin.one_seg_each = one_seg_each; fin.dc_fits = T.dc_fits;
        fin.no_sync = (b->flags & MJ_FLAG_NO_SYNC) != 0; fin.wg_lists_ok = many_ok_dri;
        fin.force = mj::opt("MJ_HUFFMAN");
        if (const char *e = mj::opt("MJ_SYNC_CHUNK")) { const int v = atoi(e); if (v >= 256 && v <= 65536 && v % 4 == 0) fin.forced_chunk = v; }
        const mj::FormChoice fc = mj::choose_stage1_form(fin);
        p->use_lanes = fc.use_lanes;
        p->sync_chunk_bytes = fc.sync_chunk_bytes;
        F.want_sync = fc.want_sync;
        if (F.want_sync && F.many_tabs) {
            // (shorter chunks = less stream per workgroup = fewer images per workgroup: if the chunk size chosen above
            // leaves some workgroup with too many tables, shorter chunks get a try)
            bool many_ok_sync = false;
            for (int cb : {p->sync_chunk_bytes, 512, 256}) {
                if (cb > p->sync_chunk_bytes) continue;
                if (wg_table_lists(S, cb, F)) { many_ok_sync = true; p->sync_chunk_bytes = cb; break; }
            }
            if (!many_ok_sync) F.want_sync = false;
        }
        if (F.want_sync) p->use_lanes = true;
    }

    // the lane forms' table lists, stage-0 stream and bit counts; the synchronisation form's chunks, states, counting tables, pieces
    int sync_layout(const BatchSegments &S, const TableRoles &T, const Forms &F) {
        const std::vector<mj::DevSegment> &segs = S.segs;
        if (!p->use_lanes) return MJ_OK;
        if (F.many_tabs) {
            if (int rc = upload(p, &p->d_wg_tabs_lanes, F.wl_lanes.data(), F.wl_lanes.size())) return rc;
            if (F.want_sync)
                if (int rc = upload(p, &p->d_wg_tabs_count, F.wl_count.data(), F.wl_count.size())) return rc;
        }
        // stage 0 output: segment i's kept bytes start at dword (begin_i >> 2) + i, so regions never overlap
        const size_t sbytes = ((size_t)b->blob_len / 4 + segs.size() + 256) * 4;
        MJ_HIP(ctx, alloc(p, &p->d_stream, sbytes));
        p->stream_bytes = sbytes;
        MJ_HIP(ctx, hipMemsetAsync(p->d_stream, 0, sbytes, ctx->setup_stream));
        MJ_HIP(ctx, alloc(p, &p->d_seg_bits, (segs.size() + 1) * sizeof(int32_t)));
        if (!F.want_sync) return MJ_OK;
        const int cb = p->sync_chunk_bytes;
        std::vector<mj::DevChunk> ck;
        for (size_t i = 0; i < segs.size(); ++i)
            for (int j = 0; j < std::max(1, (segs[i].len + cb - 1) / cb); ++j) ck.push_back(mj::DevChunk{(int32_t)i, j});
        p->n_chunks = (int64_t)ck.size();
        if (int rc = upload(p, &p->d_chunks, ck.data(), ck.size())) return rc;
        MJ_HIP(ctx, alloc(p, &p->d_stateA, ck.size() * 8 + 16));
        MJ_HIP(ctx, alloc(p, &p->d_stateB, ck.size() * 8 + 16));
        MJ_HIP(ctx, alloc(p, &p->d_couts, ck.size() * sizeof(mj::DevChunkOut) + 16));
        MJ_HIP(ctx, alloc(p, &p->d_vsegs, ck.size() * sizeof(mj::DevVSeg) + 16));
        MJ_HIP(ctx, alloc(p, &p->d_changed, (size_t)(p->sync_rounds + 8) * sizeof(int32_t)));   // [0]: round 0's, [r]: repair round r's count of changed exit states
        std::vector<int32_t> c0(segs.size() + 1, 0);      // first chunk of every restart segment: k_build_vsegs runs one workgroup per segment
        for (size_t i = 0; i < segs.size(); ++i) c0[i + 1] = c0[i] + std::max(1, (segs[i].len + cb - 1) / cb);
        if (int rc = upload(p, &p->d_seg_chunk0, c0.data(), c0.size())) return rc;
        // the counting walks on resolved tables (huffman_sync.hip: k_count) where the batch is of the everyday kind: at most
        // 8 tables, one role each, MCUs of at most 8 blocks; MJ_SYNC_COUNT = classic | resolved (tests, measurements)
        const char *e = mj::opt("MJ_SYNC_COUNT");
        bool ok = !(e && !strcmp(e, "classic")) && !F.many_tabs && !T.both_roles && b->n_huff <= 8;
        for (const mj::DevImage &im : p->h_images) ok = ok && im.blocks_per_mcu <= 8 && im.ncomp <= 3;
        int wb = 12;
        if (const char *w = mj::opt("MJ_SYNC_BITS")) wb = atoi(w);
        for (; ok && wb >= 10; --wb) {
            std::vector<uint32_t> lc;
            int tb = 0;
            if (!mj::build_count_tables(b, T.role, wb, lc, tb)) break;
            if ((size_t)tb * (size_t)b->n_huff > 150 * 1024) continue;             // a narrower index fits
            if (int rc = upload(p, &p->d_lutc, lc.data(), lc.size())) return rc;
            p->lutc_tab_bytes = tb; p->lutc_bits = wb;
            MJ_HIP(ctx, alloc(p, &p->d_sync_items, ck.size() * 16 + 16));
            break;
        }
        // stage 0 of long segments runs piece by piece (16 KiB of source bytes per wavefront)
        std::vector<mj::DevPiece> pcs;
        for (size_t i = 0; i < segs.size(); ++i) {
            const int32_t first = (int32_t)pcs.size();
            for (int off = 0; off == 0 || off < segs[i].len; off += 16384)
                pcs.push_back(mj::DevPiece{(int32_t)i, first, off, std::min(16384, std::max(0, segs[i].len - off))});
        }
        p->n_pieces = (int64_t)pcs.size();
        if (int rc = upload(p, &p->d_pieces, pcs.data(), pcs.size())) return rc;
        MJ_HIP(ctx, alloc(p, &p->d_piece_kept, pcs.size() * sizeof(int32_t) + 16));
        p->use_sync = true;
        return MJ_OK;
    }

    // the lane form deals restart segments out by length (huffman_lanes13.hip: by_length, longest first); MJ_SEG_ORDER = blob | binned | striped
    int segment_order(const BatchSegments &S, const Forms &F, std::vector<int32_t> &by_length) {
        const std::vector<mj::DevSegment> &segs = S.segs;
        if (!(p->use_lanes && !p->use_sync && p->d_lut13 && S.jobs.empty() && segs.size() > 1)) return MJ_OK;
        const char *e = mj::opt("MJ_SEG_ORDER");
        // (measured, 1024 x 1080p: files of mixed content 7.5 ms in blob order, 7.9 binned, 6.65 striped; files of one kind
        // 4.01 / 4.13 — so segments of similar length stay in blob order)
        const bool spread = mj::spread_lengths(F.seg_len.data(), (int64_t)F.seg_len.size());
        p->seg_order_mode = (e && !strcmp(e, "blob")) ? 0 : ((e && !strcmp(e, "binned")) ? 1 : ((e && !strcmp(e, "striped")) || spread ? 2 : 0));
        if (!p->seg_order_mode) return MJ_OK;
        by_length.resize(segs.size());
        for (size_t i = 0; i < segs.size(); ++i) by_length[i] = (int32_t)i;
        std::stable_sort(by_length.begin(), by_length.end(), [&](int32_t x, int32_t y) { return segs[x].len > segs[y].len; });
        return upload(p, &p->d_by_length, by_length.data(), by_length.size());
    }

    // One launch for both stages (fused.hip) where the batch allows it: the resolved-table lane form in blob order on
    // a uniform batch of 4:4:4 / 4:2:2 / 4:4:0 / 4:2:0 colour files whose restart interval is ONE MCU ROW (a producer
    // wave that is through MCU m has then finished column m of all its rows, which is the consumers' unit of work),
    // x-major pixels, no seam outputs, a stage-2 job = a whole MCU column, and LDS left for at least one consumer
    // wavefront beside the producers.  MJ_FUSED=0 keeps the two launches; MJ_FUSED_CONSUMERS bounds the consumers.
    int fused_setup(const BatchSegments &S, const TableRoles &T, const std::vector<int32_t> &by_length) {
        const int64_t n_segs = (int64_t)S.segs.size();
        int want_cons = 8, want_cons_x = 6;
        bool allow = true;
        if (const char *e = mj::opt("MJ_FUSED")) allow = atoi(e) != 0;
        if (roi_plan) allow = false;             // (window plans: stage 0, stage 1 and the window stage 2)
        if (const char *e = mj::opt("MJ_FUSED_CONSUMERS")) want_cons = want_cons_x = atoi(e);
        int luma13 = -1;                                     // MJ_FUSED_LUMA13: 0 / 1 overrides which form keeps component 0's table at 13 bits
        if (const char *e = mj::opt("MJ_FUSED_LUMA13")) luma13 = atoi(e);
        const mj::DevImage &i0 = p->h_images[0];
        mj::FusedInputs fi;
        fi.lanes_resolved = p->use_lanes && !p->use_sync && p->d_lut13 && p->n_ac13 <= 4;
        fi.seg_order_mode = p->seg_order_mode; fi.uniform = p->uniform; fi.generic = p->generic; fi.progressive = prog;
        fi.transposed = p->transposed; fi.ncomp = p->ncomp; fi.hmax = p->hmax; fi.vmax = p->vmax; fi.layout = p->layout;
        fi.flags = p->flags; fi.seam_or_exact_flags = MJ_FLAG_EXACT_ONLY | MJ_FLAG_KEEP_PLANES | MJ_FLAG_KEEP_IDCT;
        fi.restart_interval = i0.restart_interval; fi.mcu_count_h = i0.mcu_count_h; fi.mcu_count_v = i0.mcu_count_v;
        fi.jobs_per_image = p->jobs_per_image; fi.n_segs = n_segs; fi.n_images = b->n_images;
        for (const mj::DevImage &im : p->h_images) fi.same_interval = fi.same_interval && im.restart_interval == i0.restart_interval;
        const int fused_spi = (int)mj::fused_segments_per_image(fi);
        // Restart segments of very different lengths (dealt out by length, seg_order_mode 2: files of mixed content) in
        // blob order — whole images per workgroup — would let the longest wave set the pace of everything (bench.py's mixed
        // content: 11.3 ms fused that way against 10.6 as two launches): they keep their order, and the fused launch's
        // consumers take their jobs from ONE pool, handed over across workgroups (mode 2).
        const int mode = mj::fused_applies(fi);
        // A fused launch's AC tables: a 12-bit main level (half the LDS of the stage-1 kernel's 13 bits) and second-level tables
        // sized to the batch's codes.  With the segments dealt out by length (mode 2) the table of component 0 keeps 13 bits
        // where four consumers still fit beside it: the long segments of such batches are the ones with large coefficients,
        // whose symbols a 12-bit table finishes least often, and the launch lasts as long as their walk.
        // (0 = built and uploaded, 1 = such tables cannot be built — no fused launch then —, negative = an API error)
        int acb = 12, want_prod = 0;                         // MJ_FUSED_ACBITS / MJ_FUSED_PRODUCERS: the experiments of profiles/r06_fused_balance.txt
        if (const char *e = mj::opt("MJ_FUSED_ACBITS")) acb = atoi(e);
        if (const char *e = mj::opt("MJ_FUSED_PRODUCERS")) want_prod = atoi(e);
        auto fused_tables = [&](bool luma13) -> int {
            int ab[4] = {acb, acb, acb, acb};
            if (luma13) ab[(p->ac_slot_pk >> (8 * i0.tab_index[i0.blk_ac_slot[0]])) & 0xFF] = 13;
            std::vector<uint32_t> lf;
            if (!mj::build_resolved_tables(b, T.role, p->ac_slot_pk, p->n_ac13, ab, 0, lf, p->lutf_off, p->lutf_total)) return 1;
            for (int sl = 0; sl < 4; ++sl) p->lutf_bits[sl] = ab[sl];
            return upload(p, &p->d_lut12, lf.data(), lf.size());        // (a second try replaces the first one's tables)
        };
        int rc;
        if (allow && want_cons > 0 && mode == 1) {
            if ((rc = fused_tables(luma13 == 1)) < 0) return rc;
            if (rc == 0) {
                p->fused = mj::fused_shape(mj::device_cus(), p->lutf_total, p->n_dc13, p->hmax, p->vmax, p->transposed, b->n_images, fused_spi, want_cons, want_prod);
                p->fused_spi = fused_spi;
                p->use_fused = p->fused.ok;
            }
        } else if (allow && want_cons_x > 0 && mode == 2 && p->d_by_length) {
            if ((rc = fused_tables(luma13 != 0)) < 0) return rc;
            if (rc == 0) p->fused = mj::fused_shape_x(mj::device_cus(), p->lutf_total, p->n_dc13, p->hmax, p->vmax, p->transposed, n_segs, want_cons_x);
            if (rc == 1 || !p->fused.ok || p->fused.n_cons < std::min(want_cons_x, 4)) {       // (no room for them beside a 13-bit table: 12 bits all round)
                if ((rc = fused_tables(false)) < 0) return rc;
                p->fused = mj::FusedShape{};
                if (rc == 0) p->fused = mj::fused_shape_x(mj::device_cus(), p->lutf_total, p->n_dc13, p->hmax, p->vmax, p->transposed, n_segs, want_cons_x);
            }
            // (six consumers — all that fit beside a 13-bit table — not eight: with segments of very different lengths the launch
            // lasts as long as its longest wave's walk, and every consumer beside it slows that walk.  bench.py's mixed content,
            // ms per step: 12-bit tables all round 2 consumers 10.2, 4: 8.9, 6: 9.1, 8: 10.5; component 0's table at 13 bits
            // 4: 8.1-8.4, 5: 7.8-7.9, 6: 7.6-7.8; the two launches 10.4)
            p->fused_spi = fused_spi;
            if (p->fused.ok) {
                // which progress word a segment's wave reports to: the walk deals rank r of the sorted list to wave r mod waves
                const int64_t n_waves = (int64_t)p->fused.n_wg * p->fused.n_prod;
                std::vector<int32_t> holder(S.segs.size());
                for (size_t r = 0; r < by_length.size(); ++r) holder[(size_t)by_length[r]] = (int32_t)((int64_t)r % n_waves);
                if ((rc = upload(p, &p->d_holder, holder.data(), holder.size())) != MJ_OK) return rc;
                // (the ticket counters, the progress words, and room for every job on the list of jobs given up)
                const int64_t jobs_cap = (int64_t)b->n_images * std::max<int64_t>(p->jobs_per_image, (int64_t)i0.mcu_count_v * i0.mcu_count_h);
                MJ_HIP(ctx, alloc(p, &p->d_xwords, (size_t)(32 + n_waves + jobs_cap) * sizeof(uint32_t)));
                p->use_fused = true;
            }
        }
        return MJ_OK;
    }

    // the segment lists, the marker-scan jobs, a progressive batch's scans — and the blob: uploaded, the caller's, or a padded copy of it
    int resolve_blob(const BatchSegments &S, mj::ProgScans &prog_scans) {
        int rc;
        if ((rc = upload(p, &p->d_segs, S.segs.data(), S.segs.size())) != MJ_OK) return rc;
        if (!S.full_segs.empty()) {
            if ((rc = upload(p, &p->d_segs_full, S.full_segs.data(), S.full_segs.size())) != MJ_OK) return rc;
            if ((rc = upload(p, &p->d_seg_gather, S.gather.data(), S.gather.size())) != MJ_OK) return rc;
        }
        if (!S.jobs.empty()) {
            if (prog) return fail(ctx, MJ_ERR_INVALID, "MJ_FLAG_GPU_SEGMENT is for baseline batches");
            if ((rc = upload(p, &p->d_jobs, S.jobs.data(), S.jobs.size())) != MJ_OK) return rc;
            p->n_jobs = (int)S.jobs.size();
        }
        if (prog && (rc = mj::plan_progressive_upload(ctx, b, p, prog_scans)) != MJ_OK) return rc;
        if (b->blob_mem == MJ_MEM_HOST) {
            if ((rc = upload(p, &p->d_blob_owned, b->blob, (size_t)b->blob_len, 1024)) != MJ_OK) return rc;
            p->d_blob = p->d_blob_owned;
            return MJ_OK;
        }
        if (((uintptr_t)b->blob & 3) != 0) return fail(ctx, MJ_ERR_INVALID, "device blob must be 4-byte aligned");
        // the bit readers fetch up to 127 dwords past a segment's aligned start (wave_bits.h) and one dword ahead per
        // lane: a caller-owned blob must be that much longer than its last segment (uploads get the slack here)
        int64_t last_end = 0;
        for (int64_t i = 0; i < b->n_segments; ++i) last_end = b->seg_end[i] > last_end ? b->seg_end[i] : last_end;
        if (!(b->flags & MJ_FLAG_GPU_SEGMENT) && last_end + 512 > b->blob_len)
            return fail(ctx, MJ_ERR_INVALID, "device blob: blob_len must include 512 readable bytes behind the last segment");
        if (!S.jobs.empty() && ((uintptr_t)b->blob & 15) != 0)
            return fail(ctx, MJ_ERR_INVALID, "MJ_FLAG_GPU_SEGMENT: device blob must be 16-byte aligned");
        p->d_blob = b->blob;
        // MJ_FLAG_GPU_SEGMENT promises 16 readable bytes behind blob_len, which is all the marker scan and stage 0 need —
        // but a plan that ends up in the wave form (small batches, generic sampling layouts, tables in both roles) reads the
        // blob itself, up to 508 bytes behind a segment's aligned start: such a plan works on its own padded copy
        // (copied at every execute, on the execute's stream: the caller's bytes need not be there yet when the plan is made)
        if ((b->flags & MJ_FLAG_GPU_SEGMENT) && !p->use_lanes && last_end + 512 > b->blob_len) {
            MJ_HIP(ctx, alloc(p, &p->d_blob_owned, (size_t)b->blob_len + 1024 + 16));
            MJ_HIP(ctx, hipMemsetAsync(p->d_blob_owned + b->blob_len, 0, 1024, ctx->setup_stream));
            p->blob_src = b->blob; p->blob_src_len = b->blob_len;
            p->d_blob = p->d_blob_owned;
        }
        return MJ_OK;
    }

    // the coefficient store, the statuses, the seam buffers, a window plan's windows, and the plan's two events
    int output_buffers(const BatchSegments &S) {
        MJ_HIP(ctx, alloc(p, &p->d_coef, (size_t)S.blk * 64 * sizeof(int16_t) + 16));
        // (the resolved-table lane form stores every block of every MCU of every segment it is given, zeros included: no need to
        // clear 6 GB per plan first — 1.5 ms of a 1024-image plan's creation.  Only where the host listed the segments, though:
        // virtual segments of an image that did not settle, or the segments of a file whose marker count is off, do not cover
        // their image, and what a recycled buffer held before must not show through in a failed image's pixels)
        if (!(p->d_lut13 && p->use_lanes && !p->use_sync && S.jobs.empty()))
            MJ_HIP(ctx, hipMemsetAsync(p->d_coef, 0, (size_t)S.blk * 64 * sizeof(int16_t), ctx->setup_stream));
        MJ_HIP(ctx, alloc(p, &p->d_status, (size_t)b->n_images * sizeof(int32_t)));
        MJ_HIP(ctx, hipMemsetAsync(p->d_status, 0, (size_t)b->n_images * sizeof(int32_t), ctx->setup_stream));
        if (b->flags & MJ_FLAG_KEEP_PLANES) MJ_HIP(ctx, alloc(p, &p->d_planes, (size_t)S.rgb * sizeof(int16_t) + 16));
        if (b->flags & MJ_FLAG_KEEP_IDCT) MJ_HIP(ctx, alloc(p, &p->d_idct, (size_t)S.blk * 64 * sizeof(int16_t) + 16));
        if (roi_plan) {
            p->windowed = true;
            p->win_total_mcus = S.win_prefix[b->n_images];
            if (int rc = upload(p, &p->d_win, p->h_win.data(), p->h_win.size())) return rc;
            if (int rc = upload(p, &p->d_win_mcu_prefix, S.win_prefix.data(), S.win_prefix.size())) return rc;
        }
        // The clears above run on the setup stream, which neither the context stream nor a caller's stream waits for: the
        // plan's first use waits (on the host) for this event, or the tail of the 6 GB clear could land after the first
        // blocks the first execute writes.  Not waiting here lets a serving loop create the next batch's plan while this
        // context's stream is still busy with the current batch.
        MJ_HIP(ctx, hipEventCreateWithFlags(&p->ready, hipEventDisableTiming));
        MJ_HIP(ctx, hipEventRecord(p->ready, ctx->setup_stream));
        MJ_HIP(ctx, hipEventCreateWithFlags(&p->done, hipEventDisableTiming));
        return MJ_OK;
    }
};

}  // namespace

// the plain plan and the window plan (roi_plan), step by step
int mj::plan_create_common(mj_context *ctx, const mj_batch *b, const mj_roi *rois, bool roi_plan, mj_plan **out) {
    if (int rc = check_batch(ctx, b, roi_plan, out)) return rc;
    mj_plan *p = new mj_plan();
    p->ctx = ctx; p->n_images = b->n_images; p->layout = b->layout; p->flags = b->flags;
    for (int i = 0; i < b->n_images; ++i) { int h_, v_; if (!sampling_class(b->images[i], h_, v_)) p->generic = true; }
    // (the generic stage 2, like the exact-order one, writes either orientation itself: no transposed store)
    p->transposed = (b->layout & 1) == MJ_LAYOUT_ROWMAJOR && !(p->flags & MJ_FLAG_EXACT_ONLY) && !p->generic;
    struct Guard { mj_plan *p; mj_context *c; ~Guard() { c->cur = nullptr; if (p) mj_plan_destroy(p); } } guard{p, ctx};
    if (!ctx->free_arenas.empty()) { p->arena = ctx->free_arenas.back(); ctx->free_arenas.pop_back(); }
    else if (hipHostMalloc((void **)&p->arena.base, (size_t)8 << 20, hipHostMallocDefault) == hipSuccess) p->arena.cap = (size_t)8 << 20;
    else { (void)hipGetLastError(); p->arena = mj_context::Arena{}; }
    p->arena.used = 0;
    ctx->cur = p->arena.base ? &p->arena : nullptr;
    Create c{ctx, b, p, rois, roi_plan, b->blob_mem != MJ_MEM_NONE && b->blob != nullptr, false};
    c.prog = p->progressive = c.have_entropy && b->n_scans > 0;
    BatchSegments S;
    mj::ProgScans prog_scans;      // progressive batches: plan_progressive.hip
    int rc;
    if (c.prog && !b->scans) return fail(ctx, MJ_ERR_INVALID, "mj_plan_create: n_scans > 0 without scans");
    if (c.have_entropy && (b->n_huff <= 0 || !b->huff || !b->seg_begin || !b->seg_end))
        return fail(ctx, MJ_ERR_INVALID, "mj_plan_create: entropy data without Huffman tables / segment offsets");
    if ((rc = c.describe_images(S)) != MJ_OK) return rc;
    if (c.prog && (rc = mj::plan_progressive_scans(ctx, b, p, prog_scans, S.ent)) != MJ_OK) return rc;
    if ((rc = c.upload_descriptors(S)) != MJ_OK) return rc;
    if ((rc = c.stage2_jobs()) != MJ_OK) return rc;
    if (c.have_entropy) {
        TableRoles T;
        Forms F;
        std::vector<int32_t> by_length;
        if ((rc = c.lane_tables(T)) != MJ_OK) return rc;
        c.choose_forms(S, T, F);           // (with wg_table_lists where the batch has many tables)
        if ((rc = c.sync_layout(S, T, F)) != MJ_OK) return rc;
        if ((rc = c.segment_order(S, F, by_length)) != MJ_OK) return rc;
        if ((rc = c.fused_setup(S, T, by_length)) != MJ_OK) return rc;
        if ((rc = c.resolve_blob(S, prog_scans)) != MJ_OK) return rc;
    }
    if ((rc = c.output_buffers(S)) != MJ_OK) return rc;
    guard.p = nullptr;
    *out = p;
    return MJ_OK;
}

int mj::stored_windows(const PlanRequest &q, const mj_roi *rois, std::vector<mj_roi> &stored) {
    const mj_batch *b = q.b;
    stored.resize((size_t)b->n_images);
    for (int i = 0; i < b->n_images; ++i)
        if (!stored_window(q.r.orientations ? q.r.orientations[i] : 1, b->images[i].width, b->images[i].height, rois[i], &stored[(size_t)i]))
            return fail(q.ctx, MJ_ERR_INVALID, "%s: image %d: window (x=%d, y=%d, width=%d, height=%d) is empty or not inside the oriented image", kCreateFn,
                        i, rois[i].x, rois[i].y, rois[i].width, rois[i].height);
    return MJ_OK;
}

namespace {

// The affine or perspective transform of a sized request, checked against every output's oriented image (views are in place:
// normalise_views)
int check_affine(mj::PlanRequest &q) {
    const char *fn = mj::kCreateFn;
    const mj_batch *b = q.b; const mj_plan_request &r = q.r;
    const int filter = r.transform_filter;
    for (int k = 0; k < r.n_views; ++k) {
        if (r.perspective ? mj::perspective_none(r.perspective[k]) : mj::affine_none(r.affine[k])) continue;
        const mj_image_desc &im = b->images[r.views[k].image];
        const bool t = r.orientations && (mj::orient_bits(r.orientations[r.views[k].image]) & 4);
        const int w = t ? im.height : im.width, h = t ? im.width : im.height;
        if (const char *why = r.perspective ? mj::perspective_fault(r.perspective[k].a, filter, w, h) : mj::affine_fault(r.affine[k].a, filter, w, h))
            return fail(q.ctx, MJ_ERR_INVALID, "%s: %s: output %d: %s", fn, r.perspective ? "perspective" : "affine", k, why);
    }
    return MJ_OK;
}

// The views of a sized request, checked; views that are one whole image each, in order, become their absence.
// (orientations have been checked and, where all upright, dropped)
int normalise_views(mj::PlanRequest &q) {
    const char *fn = mj::kCreateFn;
    mj_context *ctx = q.ctx; const mj_batch *b = q.b; mj_plan_request &r = q.r;
    if (r.rois) return fail(ctx, MJ_ERR_INVALID, "%s: views and rois do not go together: a view names its own window", fn);
    if (r.n_views < 1 || !r.views) return fail(ctx, MJ_ERR_INVALID, "%s: views with n_views = %d (must be at least 1, with the array)", fn, r.n_views);
    if (!b->images && b->n_images > 0) return fail(ctx, MJ_ERR_INVALID, "%s: NULL argument", fn);
    std::vector<char> named((size_t)std::max(b->n_images, 0), 0);
    bool identity = r.n_views == b->n_images;
    for (int k = 0; k < r.n_views; ++k) {
        const mj_view &v = r.views[k];
        if (v.image < 0 || v.image >= b->n_images)
            return fail(ctx, MJ_ERR_INVALID, "%s: view %d: image %d outside the %d images of the batch", fn, k, v.image, b->n_images);
        mj_roi shown, stored;
        if (!mj::view_window(b, r.orientations, v, &shown, &stored))
            return fail(ctx, MJ_ERR_INVALID, "%s: view %d: window (x=%d, y=%d, width=%d, height=%d) is empty or not inside the oriented image", fn, k,
                        v.window.x, v.window.y, v.window.width, v.window.height);
        named[(size_t)v.image] = 1;
        identity = identity && v.image == k && stored.width == b->images[k].width && stored.height == b->images[k].height;
    }
    for (int i = 0; i < b->n_images; ++i)
        if (!named[(size_t)i]) return fail(ctx, MJ_ERR_INVALID, "%s: image %d: no view names it (leave it out of the batch)", fn, i);
    if (identity && !r.affine && !r.perspective) { r.views = nullptr; r.n_views = 0; }
    return MJ_OK;
}

// What every request goes through before a plan is made of it: each field checked, in this order — where several faults coincide
// the first is reported —, and each field that names its default turned into its absence, so that "the default is exactly the plan
// without the field" holds by construction: the makers never see the difference.
// (need_ctx false: mj_debug_normalise_request — everything but the context is looked at)
int normalise_request(mj::PlanRequest &q, bool need_ctx = true) {
    const char *fn = mj::kCreateFn;
    mj_context *ctx = q.ctx; const mj_batch *b = q.b; mj_plan_request &r = q.r;
    const bool sized = r.out_width != 0 || r.out_height != 0;
    // (transform_filter and transform_fill belong to whichever of the two arrays is set; set alone, they are refused below)
    const bool transform_word = r.transform_filter || r.transform_fill[0] || r.transform_fill[1] || r.transform_fill[2];
    // (n_views switches views on: an array that comes with a count of 0 is not looked at, and the makers, who test the pointer,
    // never see it)
    if (!r.n_views) r.views = nullptr;
    // the first field, in this order, that only a sized request has.  The transform is named by its array; the filter or a fill
    // byte alone, and both arrays at once — either is refused further down, where there is a size —, say "affine"
    const char *transform_name = r.perspective && !r.affine ? "perspective" : (r.affine || r.perspective || transform_word) ? "affine" : nullptr;
    const char *unsized = r.slots ? "slots" : r.output ? "output" : r.filter ? "filter" : r.places ? "places" : r.fill ? "fill"
                        : r.reducing_gap != 0 ? "reducing_gap" : r.n_views ? "views" : transform_name ? transform_name
                        : r.colour ? "colour_ops" : nullptr;
    // (what slots, the mirror flags and places have one entry for: the views of a request with views, else the images)
    const int n_out = r.n_views > 0 ? r.n_views : (b ? b->n_images : 0);
    if (!mj::resize_filter_known(r.filter)) return fail(ctx, MJ_ERR_INVALID, "%s: filter %d is none of MJ_FILTER_*", fn, r.filter);
    if (r.mode != MJ_MODE_NATIVE && r.mode != MJ_MODE_L && r.mode != MJ_MODE_RGB) return fail(ctx, MJ_ERR_INVALID, "%s: mode %d is none of MJ_MODE_*", fn, r.mode);
    if (r.mode == mj::batch_ncomp(b)) r.mode = MJ_MODE_NATIVE;      // (the files' own count)
    bool stretched = true;                                          // (every image over the whole canvas)
    for (int i = 0; r.places && b && i < n_out && stretched; ++i)
        stretched = r.places[i].width == r.out_width && r.places[i].height == r.out_height && r.places[i].x == 0 && r.places[i].y == 0;
    if (stretched) r.places = nullptr;
    bool upright = true;
    for (int i = 0; r.orientations && b && i < b->n_images; ++i) {
        if (r.orientations[i] < 1 || r.orientations[i] > 8) return fail(ctx, MJ_ERR_INVALID, "%s: image %d: orientation %d (must be 1..8)", fn, i, (int)r.orientations[i]);
        upright = upright && r.orientations[i] == 1;
    }
    if (upright) r.orientations = nullptr;
    // the output description: it needs nothing else, not even a context (the message is then mj_last_error(NULL)'s).
    // (A batch's component count is its first image's; all three entries are looked at when there is no image to ask.)
    if (r.output)
        if (const char *why = mj::output_fault(r.output->dtype, r.output->normalize != 0, r.mode ? r.mode : mj::batch_ncomp(b), r.output->mean, r.output->std))
            return fail(ctx, MJ_ERR_INVALID, "%s: output: %s", fn, why);
    // (0: no first step; else Pillow's rule, and its message)
    if (r.reducing_gap != 0 && !(std::isfinite(r.reducing_gap) && r.reducing_gap >= 1.0))
        return fail(ctx, MJ_ERR_INVALID, "%s: reducing_gap must be 1.0 or greater (or 0: none)", fn);
    if (!ctx && need_ctx) return MJ_ERR_INVALID;
    if (!b || !q.out) return fail(ctx, MJ_ERR_INVALID, "%s: NULL argument", fn);
    *q.out = nullptr;
    if (!sized && unsized) return fail(ctx, MJ_ERR_INVALID, "%s: %s needs a size (out_width, out_height)", fn, unsized);
    if (sized && (r.out_width < 1 || r.out_height < 1 || r.out_width > 65535 || r.out_height > 65535))
        return fail(ctx, MJ_ERR_INVALID, "%s: output size %d x %d (both must be 1..65535)", fn, r.out_width, r.out_height);
    // (a window plan's refusal of the KEEP flags is plan_create_common's)
    if ((sized || r.orientations || r.mode) && (b->flags & (MJ_FLAG_KEEP_PLANES | MJ_FLAG_KEEP_IDCT)))
        return fail(ctx, MJ_ERR_INVALID, sized ? "%s: the seam outputs (MJ_FLAG_KEEP_PLANES / MJ_FLAG_KEEP_IDCT) are at the files' own sizes; a resized plan has none"
                                               : "%s: the seam outputs (MJ_FLAG_KEEP_PLANES / MJ_FLAG_KEEP_IDCT) are in stored order; an oriented plan has none", fn);
    if (r.colour) {      // (every chain checked; all of them empty: the request without the field)
        bool none = true;
        for (int k = 0; k < n_out; ++k) {
            if (const char *why = mj::colour_fault(r.colour[k])) return fail(ctx, MJ_ERR_INVALID, "%s: colour_ops: output %d: %s", fn, k, why);
            none = none && r.colour[k].n == 0;
        }
        if (none) r.colour = nullptr;
    }
    if (r.affine && r.perspective) return fail(ctx, MJ_ERR_INVALID, "%s: affine and perspective do not go together", fn);
    if (r.affine || r.perspective) {
        const int n_out_af = r.n_views > 0 ? r.n_views : b->n_images;
        if (r.transform_filter != MJ_AFFINE_NEAREST && r.transform_filter != MJ_AFFINE_BILINEAR && r.transform_filter != MJ_AFFINE_BICUBIC)
            return fail(ctx, MJ_ERR_INVALID, "%s: affine: filter %d is none of MJ_AFFINE_*", fn, r.transform_filter);
        bool none = true;
        for (int k = 0; k < n_out_af && none; ++k) none = r.perspective ? mj::perspective_none(r.perspective[k]) : mj::affine_none(r.affine[k]);
        if (none) {       // (no output is transformed: the request without the field)
            r.affine = nullptr; r.perspective = nullptr; r.transform_filter = 0;
            r.transform_fill[0] = r.transform_fill[1] = r.transform_fill[2] = 0;
        }
    } else if (transform_word) {
        return fail(ctx, MJ_ERR_INVALID, "%s: transform_filter / transform_fill without an array (affine or perspective)", fn);
    }
    const bool transform = r.affine || r.perspective;
    if (transform) {
        if (r.reducing_gap != 0)
            return fail(ctx, MJ_ERR_INVALID, "%s: %s and reducing_gap do not go together yet: the reduce launch would have to read the transformed images", fn,
                        r.perspective ? "perspective" : "affine");
        if (!b->images && b->n_images > 0) return fail(ctx, MJ_ERR_INVALID, "%s: NULL argument", fn);
        if (!r.n_views) {       // (windows, or whole images, as one view per image: the plan decodes whole images)
            q.own_views.resize((size_t)b->n_images);
            for (int i = 0; i < b->n_images; ++i) q.own_views[(size_t)i] = mj_view{i, r.rois ? r.rois[i] : mj_roi{0, 0, 0, 0}};
            if (b->n_images > 0) { r.views = q.own_views.data(); r.n_views = b->n_images; r.rois = nullptr; }
        }
    }
    if (r.n_views)
        if (int rc = normalise_views(q)) return rc;
    if (transform && r.n_views)
        if (int rc = check_affine(q)) return rc;
    const int n_outputs = r.n_views ? r.n_views : b->n_images;
    if (!r.slots) r.n_slots = n_outputs;
    for (int i = 0; r.slots && i < n_outputs; ++i)
        if (r.slots[i] < 0 || r.slots[i] >= r.n_slots)
            return fail(ctx, MJ_ERR_INVALID, "%s: %s %d: slot %d outside the %d slots of the output", fn, r.n_views ? "view" : "image", i, r.slots[i], r.n_slots);
    // (no image with a factor above 1: there is no first step, and the plan is the plan without the field)
    if (r.reducing_gap != 0 && !mj::reduce_applies(b, r)) r.reducing_gap = 0;
    return MJ_OK;
}

}  // namespace

extern "C" {

int mj_debug_fused_applies(int32_t layout, int32_t ncomp, int32_t hmax, int32_t vmax, int32_t mcus_per_row, int32_t mcu_rows,
                           int32_t restart_interval, int32_t n_images, uint32_t traits, uint32_t flags, int32_t *mode_out) {
    if (!mode_out || mcus_per_row < 1 || mcu_rows < 1 || n_images < 1) return MJ_ERR_INVALID;
    mj::FusedInputs f;
    f.lanes_resolved = !(traits & 1u); f.seg_order_mode = (traits & 2u) ? 2 : ((traits & 4u) ? 1 : 0);
    f.uniform = !(traits & 8u); f.generic = (traits & 16u) != 0; f.progressive = (traits & 32u) != 0; f.same_interval = !(traits & 64u);
    f.layout = layout; f.transposed = (layout & 1) != 0; f.ncomp = ncomp; f.hmax = hmax; f.vmax = vmax;
    f.flags = flags; f.seam_or_exact_flags = MJ_FLAG_EXACT_ONLY | MJ_FLAG_KEEP_PLANES | MJ_FLAG_KEEP_IDCT;
    f.restart_interval = restart_interval; f.mcu_count_h = mcus_per_row; f.mcu_count_v = mcu_rows;
    f.jobs_per_image = mcus_per_row;        // (x-major plans number their jobs column by column, whole or in equal pieces)
    f.n_images = n_images; f.n_segs = (int64_t)n_images * mj::fused_segments_per_image(f);
    *mode_out = mj::fused_applies(f);
    return MJ_OK;
}

int mj_debug_stage1_form(const int32_t *seg_len, int64_t n_segs, uint64_t blob_len, int32_t n_huff, uint32_t traits, const char *force,
                         int32_t forced_chunk, int32_t out[4]) {
    if (!out || (n_segs > 0 && !seg_len) || n_segs < 0) return MJ_ERR_INVALID;
    mj::FormInputs in;
    in.seg_len = seg_len; in.n_segs = n_segs; in.blob_len = blob_len; in.n_huff = n_huff;
    in.both_roles = traits & 1; in.ordered = !(traits & 2); in.progressive = traits & 4; in.generic = traits & 8;
    in.gpu_segment = traits & 16; in.one_seg_each = traits & 32; in.dc_fits = !(traits & 64); in.no_sync = traits & 128;
    in.wg_lists_ok = !(traits & 256);
    in.force = (force && force[0]) ? force : nullptr;
    in.forced_chunk = forced_chunk;
    const mj::FormChoice c = mj::choose_stage1_form(in);
    out[0] = in.progressive ? MJ_FORM_SCANS : ((c.want_sync ? MJ_FORM_SYNC : (c.use_lanes ? MJ_FORM_LANES : MJ_FORM_WAVE)) | (c.many_tabs && (c.want_sync || c.use_lanes) ? MJ_FORM_WG_TABLES : 0));
    out[1] = c.sync_chunk_bytes;
    out[2] = (int32_t)std::min<int64_t>(c.est_chunks, 0x7fffffff);
    out[3] = mj::spread_lengths(seg_len, n_segs) ? 1 : 0;
    return MJ_OK;
}

int mj_debug_normalise_request(const mj_batch *b, const mj_plan_request *request, mj_plan_request *normal) {
    if (!normal) return MJ_ERR_INVALID;
    mj_plan *none = nullptr;
    mj::PlanRequest q{nullptr, b, &none, request ? *request : mj_plan_request{}};
    const int rc = normalise_request(q, false);
    if (rc == MJ_OK) *normal = q.r;
    if (rc == MJ_OK && !q.own_views.empty()) normal->views = nullptr;      // (the library's own views end with q: the count alone goes out)
    return rc;
}

int mj_plan_create_with(mj_context *ctx, const mj_batch *b, const mj_plan_request *request, mj_plan **out) {
    mj::PlanRequest q{ctx, b, out, request ? *request : mj_plan_request{}};
    if (int rc = normalise_request(q)) return rc;
    if (q.r.out_width) return mj::create_resized(q);
    if (q.r.orientations || q.r.mode) return mj::create_oriented(q);
    return mj::plan_create_common(ctx, b, q.r.rois, q.r.rois != nullptr, out);
}

int mj_plan_create(mj_context *ctx, const mj_batch *b, mj_plan **out) { return mj_plan_create_with(ctx, b, nullptr, out); }

int mj_plan_derive(mj_plan *parent, const mj_batch *b, const mj_plan_request *request, mj_plan **out) {
    const char *fn = "mj_plan_derive";
    if (!parent) return fail(nullptr, MJ_ERR_INVALID, "%s: NULL argument", fn);
    mj_context *ctx = parent->ctx;
    if (!b || !request || !out) return fail(ctx, MJ_ERR_INVALID, "%s: NULL argument", fn);
    *out = nullptr;
    if (parent->derived) return fail(ctx, MJ_ERR_INVALID, "%s: the parent is itself derived (derive from the plan that decodes)", fn);
    if (!parent->resized || parent->orient_only)
        return fail(ctx, MJ_ERR_INVALID, "%s: the parent has no size (out_width, out_height): only a sized plan keeps its decoded images", fn);
    if (parent->windowed) return fail(ctx, MJ_ERR_INVALID, "%s: the parent is a window plan: it does not decode whole images", fn);
    // the batch is the parent's: what the stage builders read of it — image count, sizes, component counts, the layout — is checked
    bool same = b->n_images == parent->n_images && b->layout == parent->layout && (b->images || b->n_images <= 0);
    for (int i = 0; same && i < b->n_images; ++i)
        same = b->images[i].width == parent->h_images[i].width && b->images[i].height == parent->h_images[i].height && b->images[i].ncomp == parent->h_images[i].ncomp;
    if (!same) return fail(ctx, MJ_ERR_INVALID, "%s: the batch is not the one the parent was made from (image count, sizes, components, layout)", fn);
    if (!request->out_width && !request->out_height) return fail(ctx, MJ_ERR_INVALID, "%s: the request needs a size (out_width, out_height)", fn);
    if (request->rois) return fail(ctx, MJ_ERR_INVALID, "%s: rois: a derived plan's windows are views", fn);
    mj::PlanRequest q{ctx, b, out, *request};
    if (int rc = normalise_request(q)) return rc;
    MJ_HIP(ctx, hipSetDevice(ctx->device));
    return mj::create_derived(q, parent);
}

}  // extern "C"
