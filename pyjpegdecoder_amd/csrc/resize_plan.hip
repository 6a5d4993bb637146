// Plan creation for the resized plans (a mj_plan_request with a size): host code only.  The tap tables' arithmetic
// (build_resize_axis), the kernels, launch_resize and build_normalize_table are resize.hip's; this file decides what they are
// given.  create_resized takes the normalised request (plan.h: PlanRequest) and goes through it in named steps:
//   placed_source_ranges   placed plans: what every image's axes need of their source, and the window plan derived from that
//   reduce_stage           reducing plans: every image's factors, phases, reduced size and float32 box, and the reduce launch's records
//   TapTables              one table per distinct axis, range-checked, reversed for orientations, serialised for the kernels
//   choose_tile            the tile a workgroup takes and where its parts lie in LDS — a pure function of the tables and sizes
//   output_table           the 256 x C elements a 2- or 4-byte output looks its bytes up in
// A request with views (mj_plan_request.views) goes the same way with one record per VIEW in the resize and reduce launches: the
// plan is the plain plan of the images, a view's record starts at its window's origin inside its decoded image (pixel_offset), keeps
// that image's row as its pitch, and its tables — and factors — are its window's.
// A request with an affine transform (mj_plan_request.affine; always with views, see plan.h) adds one step,
//   affine_stage           one record per output for the affine launch (affine.hip), its NEAREST index tables, and where every
//                          output's window of its transformed image lies in the plan's second buffer
// and the resize launch's records are then upright images of the output's components in THAT buffer, the window's row their pitch.
// A request with colour operations (mj_plan_request.colour) adds one step behind everything else,
//   colour_stage           the resize launch is made for uint8 canvases of the plan's own, unmirrored, canvas k for output k; the
//                          colour launches (colour.hip) get the chains, the slots, the mirror flags and the output table
#include <math.h>
#include <map>

#include "plan.h"

namespace {

struct AxisHost {
    std::vector<int32_t> lo, cnt;
    int ks = 0, word_off = 0, in_size = 0;
    // the most source entries a tile of `tile` outputs needs
    int span(int tile) const {
        int m = 0, out = (int)lo.size();
        for (int o0 = 0; o0 < out; o0 += tile) {
            int hi = 0;
            for (int o = o0; o < std::min(o0 + tile, out); ++o) hi = std::max(hi, lo[o] + cnt[o]);
            m = std::max(m, hi - lo[o0]);
        }
        return m;
    }
};

int round16(int64_t v) { return (int)((v + 15) & ~(int64_t)15); }
// bytes from the start of a decoded image — stored width x height, C interleaved components, in the plan's layout — to its pixel (x, y)
int64_t pixel_offset(int layout, int width, int height, int C, int x, int y) {
    return ((layout & 1) ? (int64_t)y * width + x : (int64_t)x * height + y) * C;
}
int dtype_size(int dtype) { return dtype == MJ_DTYPE_U8 ? 1 : dtype == MJ_DTYPE_F32 ? 4 : 2; }

}  // namespace

// what mj_plan_request.output and mj_host_normalize_table refuse: nullptr when the description is fine, else the reason
const char *mj::output_fault(int dtype, bool normalize, int ncomp, const float *mean, const float *std) {
    if (dtype != MJ_DTYPE_U8 && dtype != MJ_DTYPE_F16 && dtype != MJ_DTYPE_BF16 && dtype != MJ_DTYPE_F32) return "dtype is none of MJ_DTYPE_U8 / F16 / BF16 / F32";
    if (!normalize) return nullptr;
    if (dtype == MJ_DTYPE_U8) return "normalize needs a float dtype (MJ_DTYPE_U8 stores the resized bytes)";
    for (int c = 0; c < ncomp; ++c) {
        if (!std::isfinite(mean[c])) return "mean must be finite";
        if (!std::isfinite(std[c]) || !(std[c] > 0.0f)) return "std must be finite and > 0";
    }
    return nullptr;
}

namespace {
using mj::PlanRequest;

// ---- placed plans: the source ranges -------------------------------------------------------------------------------------
// What every axis of every image needs of its source — the taps of the canvas entries the image covers reach source entries
// [x0, x0 + nx) x [y0, y0 + ny) of the oriented image or window, whose size is sw x sh (what the tables are made for).
struct Need { int x0, nx, y0, ny, sw, sh; };
// In: the request, with its orientations (NULL: none) and windows (NULL: whole images) or views.  Out: `need`, one per output (image,
// or view — whose windows are never derived: its image is decoded whole, once, for all its views), and `derived` —
// where the ranges are less than the whole and the rule below says so, the windows of those ranges, as if the caller had asked
// for them (the plan becomes a window plan: restart segments and MCUs outside are skipped as for a caller's windows, and
// the tables are rebased to the range); else empty, and every range starts at 0 (tables over the whole image or window).
// (may_window false — a derived plan, whose decode is its parent's: the ranges are never made windows)
int placed_source_ranges(const PlanRequest &q, bool may_window, std::vector<Need> &need, std::vector<mj_roi> &derived) {
    const mj_batch *b = q.b;
    const char *fn = mj::kCreateFn;
    const mj_roi *rois = q.r.rois; const uint8_t *orient = q.r.orientations; const mj_place *places = q.r.places;
    const int filter = q.r.filter, out_width = q.r.out_width, out_height = q.r.out_height;
    const mj_view *views = q.r.views;
    const int n_out = views ? q.r.n_views : b->n_images;
    const char *what = views ? "view" : "image";
    if (!b->images && b->n_images > 0) return fail(q.ctx, MJ_ERR_INVALID, "%s: NULL argument", fn);
    need.resize((size_t)n_out);
    int64_t area_need = 0, area_all = 0;
    std::map<std::vector<int>, std::pair<int, int>> spans;      // (a batch of one size and one placement: one table per axis)
    // the source entries [*first, *first + *len) the canvas takes of an axis in_size -> resized at offset off
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
    // (the oriented image, or the caller's window of it)
    auto whole = [&](int i) {
        const int bits = orient ? mj::orient_bits(orient[i]) : 0;
        int W = b->images[i].width, H = b->images[i].height;
        if (bits & 4) std::swap(W, H);
        return mj_roi{0, 0, W, H};
    };
    for (int k = 0; k < n_out; ++k) {
        const int i = views ? views[k].image : k;
        const mj_place &pl = places[k];
        if (pl.width < 1 || pl.height < 1 || pl.width > 65535 || pl.height > 65535 || pl.x < -65535 || pl.x > 65535 || pl.y < -65535 || pl.y > 65535)
            return fail(q.ctx, MJ_ERR_INVALID, "%s: %s %d: place (width=%d, height=%d, x=%d, y=%d): the size must be 1..65535, the offsets within +-65535",
                        fn, what, k, pl.width, pl.height, pl.x, pl.y);
        if (pl.x >= out_width || pl.y >= out_height || (int64_t)pl.x + pl.width <= 0 || (int64_t)pl.y + pl.height <= 0)
            return fail(q.ctx, MJ_ERR_INVALID, "%s: %s %d: a %d x %d image at (%d, %d) does not meet the %d x %d canvas", fn, what, k, pl.width, pl.height,
                        pl.x, pl.y, out_width, out_height);
        const int W = whole(i).width, H = whole(i).height;
        mj_roi r = rois ? rois[k] : whole(i), tmp;
        if (views) mj::view_window(b, orient, views[k], &r, &tmp);      // (checked by the request's normalisation)
        Need &nd = need[(size_t)k] = Need{0, r.width, 0, r.height, r.width, r.height};
        // (a window the plan will refuse, or a size no table is built for: left as it is, for the code that refuses it)
        if (W < 1 || H < 1 || W > 65535 || H > 65535 || !mj::stored_window(1, W, H, r, &tmp)) { area_all += 1; area_need += 1; continue; }
        // (a reducing plan decodes whole images and windows as given — a shrunk window would move the cell grid — and its tables
        // are made for the reduced sizes: reduce_stage sets `need`)
        if (q.r.reducing_gap != 0) continue;
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
    if (q.r.reducing_gap != 0 || views || !may_window) derive = false;
    if (derive && area_need < area_all) {
        derived.resize((size_t)b->n_images);
        for (int i = 0; i < b->n_images; ++i) {
            const mj_roi r = rois ? rois[i] : whole(i);
            const Need &nd = need[(size_t)i];
            derived[(size_t)i] = mj_roi{r.x + nd.x0, r.y + nd.y0, nd.nx, nd.ny};
        }
    } else {
        for (Need &nd : need) nd.x0 = nd.y0 = 0;
    }
    return MJ_OK;
}

// ---- reducing plans: the first step's geometry ------------------------------------------------------------------------------
// One image, in the oriented image's axes (before its flips): the factors, the reduced size, and the part of the reduced image
// the resample reads — Pillow's box (0, 0, w / fx, h / fy), which it carries as 32-bit floats: {in0, in1} per axis.
struct Reduced { int fx, fy, w, h; float bx[2], by[2]; int64_t off; };      // (off: bytes, into the buffer of reduced images)
// In: the plan (its images' or windows' stored sizes), the request, whether the orientations exchange width and height.  Out:
// `red`, one per image — per view, in a request with views: a view has its own factors and phases, from ITS window's size and
// target, its cell grid starts at its window's origin, and its record reads its window of the decoded image (pitch: that image's
// row) —; the plan's reduce launch (p->rd, its records uploaded) and what mj_debug_reduce_shape reports; *bytes,
// the packed reduced images' size.  ALL images go through the launch: a 1 x 1 cell is the identity.
int reduce_stage(const PlanRequest &q, mj_plan *p, bool swapped, bool luma, std::vector<Reduced> &red, int64_t *bytes) {
    const char *fn = mj::kCreateFn;
    const uint8_t *orient = q.r.orientations; const mj_place *places = q.r.places;
    const mj_view *views = q.r.views;
    const int n = views ? q.r.n_views : p->n_images, CO = luma ? 1 : p->ncomp;
    // (how the source is read, as launch_resize has it: transposing orientations read the other layout's way, so in the oriented
    // image's axes an image is rows x len = w x h of an x-major reading and h x w of a row-major one)
    const bool xmajor = ((p->layout & 1) == 0) != swapped;
    std::vector<mj::DevReduceImage> recs((size_t)n);
    red.resize((size_t)n); p->h_rd.resize((size_t)n);
    mj::ReduceArgs &a = p->rd = mj::ReduceArgs{};
    a.tile_slow = 8;
    int max_slow = 1, max_fast = 1;      // the largest reduced image's rows and pixels of a row
    int64_t off = 0;
    for (int k = 0; k < n; ++k) {
        const int i = views ? views[k].image : k;
        int w = p->windowed ? p->h_win[i].w : p->h_images[i].width, h = p->windowed ? p->h_win[i].h : p->h_images[i].height;
        const int bits = orient ? mj::orient_bits(orient[i]) : 0;
        if (bits & 4) std::swap(w, h);
        // (a view: the oriented window is what is reduced; the whole oriented image gives the pitch)
        const int whole_w = w, whole_h = h;
        mj_roi shown{}, stored{};
        if (views) { mj::view_window(q.b, orient, views[k], &shown, &stored); w = shown.width; h = shown.height; }
        Reduced &r = red[(size_t)k];
        mj::reduce_factors(w, h, places ? places[k].width : q.r.out_width, places ? places[k].height : q.r.out_height, q.r.reducing_gap, &r.fx, &r.fy);
        if ((int64_t)r.fx * r.fy > mj::kReduceMaxCell)
            return fail(q.ctx, MJ_ERR_UNSUPPORTED, "%s: %s %d: reducing %d x %d by %d x %d takes cells of more than %d pixels", fn, views ? "view" : "image", k, w, h,
                        r.fx, r.fy, mj::kReduceMaxCell);
        r.w = (w + r.fx - 1) / r.fx; r.h = (h + r.fy - 1) / r.fy;
        r.bx[0] = r.by[0] = 0.0f;
        r.bx[1] = (float)((double)w / r.fx); r.by[1] = (float)((double)h / r.fy);
        // (an axis the orientation reverses: the partial cell comes first)
        const int phx = (bits & 1) ? w % r.fx : 0, phy = (bits & 2) ? h % r.fy : 0;
        mj::DevReduceImage &d = recs[(size_t)k];
        if (xmajor) mj::reduce_record(w, h, r.fx, r.fy, phx, phy, &d);
        else mj::reduce_record(h, w, r.fy, r.fx, phy, phx, &d);
        d.src_off = p->h_images[i].rgb_off; d.dst_off = r.off = off;
        if (views) {
            d.pitch = xmajor ? whole_h : whole_w;
            d.src_off += pixel_offset(p->layout, p->h_images[i].width, p->h_images[i].height, p->ncomp, stored.x, stored.y);
        }
        off += (int64_t)r.w * r.h * CO;
        max_slow = std::max(max_slow, xmajor ? r.w : r.h); max_fast = std::max(max_fast, xmajor ? r.h : r.w);
        // (mj_debug_reduce_shape: in the stored image's axes)
        if (bits & 4) p->h_rd[(size_t)k] = {r.fy, r.fx, phy, phx, r.h, r.w};
        else p->h_rd[(size_t)k] = {r.fx, r.fy, phx, phy, r.w, r.h};
    }
    // (rows cut into equal tiles, none longer than a wavefront's row of reduced bytes)
    const int cap = mj::reduce_tile_fast(CO);
    a.tiles_fast = (max_fast + cap - 1) / cap; a.tile_fast = (max_fast + a.tiles_fast - 1) / a.tiles_fast;
    a.tiles_slow = (max_slow + a.tile_slow - 1) / a.tile_slow;
    if ((int64_t)n * a.tiles_slow * a.tiles_fast > mj::kResizeGridX * (int64_t)65535)
        return fail(q.ctx, MJ_ERR_UNSUPPORTED, "%s: %lld reduce tiles are more than one launch takes; split the batch", fn, (long long)n * a.tiles_slow * a.tiles_fast);
    a.n_images = n;
    if (int rc = upload(p, &p->d_rd_images, recs.data(), recs.size())) return rc;
    a.images = p->d_rd_images;
    *bytes = off;
    return MJ_OK;
}

// ---- plans with an affine transform: the launch in front of the resize ----------------------------------------------------------
// In: the request (views in place, matrices checked), the plan, CO — the components the launch writes.  Out: the plan's affine
// launch (p->af, records and tables uploaded), `off` — per output, where its window lies in the buffer of transformed windows —
// and *bytes, that buffer's size.
// (a perspective transform — q.r.perspective — has records of its own and no tables: p->pf, and p->perspective says so)
int affine_stage(const PlanRequest &q, mj_plan *p, int CO, std::vector<int64_t> &off, int64_t *bytes) {
    const char *fn = mj::kCreateFn;
    const uint8_t *orient = q.r.orientations;
    const int n = q.r.n_views, filter = q.r.transform_filter;
    std::vector<mj::DevAffineImage> recs(q.r.perspective ? 0 : (size_t)n);
    std::vector<mj::DevPerspectiveImage> precs(q.r.perspective ? (size_t)n : 0);
    std::vector<int32_t> tabs;
    off.resize((size_t)n);
    const bool rowmajor = (p->layout & 1) != 0;
    int max_slow = 1, max_fast = 1;
    int64_t at = 0;
    // what both kinds of record say of output k: its image, orientation and window, and where its window goes
    auto place = [&](int k, auto &d) {
        const int i = q.r.views[k].image;
        mj_roi shown, stored;
        mj::view_window(q.b, orient, q.r.views[k], &shown, &stored);      // (checked by the request's normalisation)
        d.src_off = p->h_images[i].rgb_off; d.dst_off = off[(size_t)k] = at;
        d.sw = p->h_images[i].width; d.sh = p->h_images[i].height;
        d.obits = orient ? mj::orient_bits(orient[i]) : 0;
        d.w = (d.obits & 4) ? d.sh : d.sw; d.h = (d.obits & 4) ? d.sw : d.sh;
        d.x0 = shown.x; d.y0 = shown.y; d.win_w = shown.width; d.win_h = shown.height;
        at += (int64_t)d.win_w * d.win_h * CO;
        max_fast = std::max(max_fast, rowmajor ? d.win_w : d.win_h); max_slow = std::max(max_slow, rowmajor ? d.win_h : d.win_w);
    };
    for (int k = 0; k < n; ++k) {
        if (q.r.perspective) {
            mj::DevPerspectiveImage &d = precs[(size_t)k] = mj::DevPerspectiveImage{};
            place(k, d);
            const mj_perspective &m = q.r.perspective[k];
            if (!mj::perspective_none(m)) {
                d.kind = mj::perspective_kind(filter);
                for (int t = 0; t < 8; ++t) d.c[t] = m.a[t];
            }
            continue;
        }
        mj::DevAffineImage &d = recs[(size_t)k] = mj::DevAffineImage{};
        place(k, d);
        const mj_affine &m = q.r.affine[k];
        if (!mj::affine_none(m)) {
            d.kind = mj::affine_kind(m.a, filter);
            for (int t = 0; t < 6; ++t) d.a[t] = m.a[t];
            if (d.kind == 2) mj::affine_fixed(m.a, d.fx);
            if (d.kind == 1) {
                d.xtab = (int32_t)tabs.size(); d.ytab = d.xtab + d.win_w;
                tabs.resize(tabs.size() + (size_t)d.win_w + d.win_h);
                mj::affine_scale_table(m.a[0], m.a[2], d.w, d.x0, d.win_w, tabs.data() + d.xtab);
                mj::affine_scale_table(m.a[4], m.a[5], d.h, d.y0, d.win_h, tabs.data() + d.ytab);
                if (tabs.size() > ((size_t)1 << 28)) return fail(q.ctx, MJ_ERR_UNSUPPORTED, "%s: the index tables of this batch are too large", fn);
            }
        }
    }
    const int tiles_fast = (max_fast + mj::kAffineTileFast - 1) / mj::kAffineTileFast, tiles_slow = (max_slow + mj::kAffineTileSlow - 1) / mj::kAffineTileSlow;
    if ((int64_t)n * tiles_slow * tiles_fast > mj::kResizeGridX * (int64_t)65535)
        return fail(q.ctx, MJ_ERR_UNSUPPORTED, "%s: %lld affine tiles are more than one launch takes; split the batch", fn, (long long)n * tiles_slow * tiles_fast);
    uint32_t fill = 0;
    for (int c = 0; c < CO; ++c) fill |= (uint32_t)q.r.transform_fill[c] << (8 * c);
    *bytes = at;
    if (q.r.perspective) {
        mj::PerspectiveArgs &a = p->pf = mj::PerspectiveArgs{};
        a.tiles_fast = tiles_fast; a.tiles_slow = tiles_slow; a.n_images = n; a.layout = p->layout; a.fill = fill;
        if (int rc = upload(p, &p->d_pf_images, precs.data(), precs.size())) return rc;
        a.images = p->d_pf_images;
        p->perspective = true;
        return MJ_OK;
    }
    mj::AffineArgs &a = p->af = mj::AffineArgs{};
    a.tiles_fast = tiles_fast; a.tiles_slow = tiles_slow; a.n_images = n; a.layout = p->layout; a.fill = fill;
    if (int rc = upload(p, &p->d_af_images, recs.data(), recs.size())) return rc;
    if (int rc = upload(p, &p->d_af_tabs, tabs.data(), tabs.size())) return rc;
    a.images = p->d_af_images; a.tabs = p->d_af_tabs;
    return MJ_OK;
}

// ---- plans with colour operations: the launches behind the resize ---------------------------------------------------------------
// In: the request (chains checked, some not empty), the plan — its resize launch made for uint8 canvases, output k at canvas k —,
// CO — the output's components — and the output's element size.  Out: the plan's colour launches (p->co): one record per output
// with its chain, its slot's offset in elements and its mirror flag; per step, the outputs that take a histogram and, behind them
// in the same array, the outputs that are blurred and then those of the hue launch; the two canvases, the histograms, the tables and the output table, all
// plan-owned.  A plan with a blur whose canvas LDS does not hold (or under option MJ_BLUR=passes) owns a third canvas.
std::vector<uint8_t> output_table(const mj_output_desc &o, int CO, int esize);
int colour_stage(const PlanRequest &q, mj_plan *p, int CO, int out_esize) {
    const mj_plan_request &r = q.r;
    const int n = r.n_views ? r.n_views : p->n_images;
    const int64_t npix = (int64_t)r.out_width * r.out_height, canvas = (int64_t)n * npix * CO;
    mj::ColourArgs &a = p->co = mj::ColourArgs{};
    mj::ColourBlurArgs &b = p->co_blur = mj::ColourBlurArgs{};
    mj::ColourHueArgs &h = p->co_hue = mj::ColourHueArgs{};
    std::vector<mj::DevColourOutput> recs((size_t)n);
    std::vector<int32_t> list;
    std::vector<uint32_t> weights((size_t)n * 8, 0);
    for (int k = 0; k < n; ++k) {
        const mj_colour_chain &c = q.r.colour[k];
        mj::DevColourOutput &d = recs[(size_t)k] = mj::DevColourOutput{};
        d.dst_off = (int64_t)(r.slots ? r.slots[k] : k) * npix * CO;
        d.n = c.n; d.mirror = r.output && r.output->mirror && r.output->mirror[k] ? 1 : 0;
        for (int s = 0; s < c.n; ++s) {
            d.kind[s] = c.op[s].kind; d.value[s] = c.op[s].value; d.ivalue[s] = mj::colour_ivalue(c.op[s]);
            if (mj::colour_is_table(d.kind[s])) a.tables_at |= 1 << s;
            if (mj::colour_is_blur(d.kind[s])) {
                const mj::BlurPass pass = mj::colour_blur_pass(c.op[s]);
                weights[((size_t)k * 4 + s) * 2] = pass.ww; weights[((size_t)k * 4 + s) * 2 + 1] = pass.fw;
                b.passes[s] = std::max(b.passes[s], 2 * mj::colour_blur_passes(d.kind[s]));
            }
        }
        a.steps = std::max(a.steps, c.n);
    }
    for (int s = 0; s < MJ_COLOUR_MAX_OPS; ++s) {
        a.hist_first[s] = (int32_t)list.size();
        for (int k = 0; k < n; ++k)
            if (s < recs[(size_t)k].n && mj::colour_needs_hist(recs[(size_t)k].kind[s])) list.push_back(k);
    }
    a.hist_first[MJ_COLOUR_MAX_OPS] = (int32_t)list.size();
    for (int s = 0; s < MJ_COLOUR_MAX_OPS; ++s) {
        b.first[s] = (int32_t)list.size();
        for (int k = 0; k < n; ++k)
            if (s < recs[(size_t)k].n && mj::colour_is_blur(recs[(size_t)k].kind[s])) list.push_back(k);
    }
    b.first[MJ_COLOUR_MAX_OPS] = (int32_t)list.size();
    const bool blurs = b.first[MJ_COLOUR_MAX_OPS] > b.first[0];
    for (int s = 0; s < MJ_COLOUR_MAX_OPS; ++s) {
        h.first[s] = (int32_t)list.size();
        for (int k = 0; k < n; ++k)
            if (CO == 3 && s < recs[(size_t)k].n && recs[(size_t)k].kind[s] == MJ_COLOUR_ADJUST_HUE) list.push_back(k);
    }
    h.first[MJ_COLOUR_MAX_OPS] = (int32_t)list.size();
    const bool hues = h.first[MJ_COLOUR_MAX_OPS] > h.first[0];
    const char *route = mj::opt("MJ_BLUR");
    if (blurs && !(route && !strcmp(route, "passes")) && mj::blur_lds_bytes(r.out_width, r.out_height) <= mj::kBlurLdsMax)
        b.lds = (int32_t)mj::blur_lds_bytes(r.out_width, r.out_height);
    const int64_t per_output = std::max<int64_t>({(npix + mj::kColourHistPixels - 1) / mj::kColourHistPixels, (npix + 255) / 256, (int64_t)CO});
    if ((int64_t)n * per_output > mj::kResizeGridX * (int64_t)65535)
        return fail(q.ctx, MJ_ERR_UNSUPPORTED, "%s: %lld colour workgroups are more than one launch takes; split the batch", mj::kCreateFn, (long long)n * per_output);
    if (int rc = upload(p, &p->d_co_outputs, recs.data(), recs.size())) return rc;
    if (int rc = upload(p, &p->d_co_list, list.data(), list.size())) return rc;
    MJ_HIP(q.ctx, alloc(p, &p->d_canvas, (size_t)(2 * canvas) + 64));
    MJ_HIP(q.ctx, alloc(p, &p->d_co_hist, (size_t)n * 1024 * sizeof(uint32_t)));
    MJ_HIP(q.ctx, alloc(p, &p->d_co_tables, (size_t)n * 768));
    if (blurs)
        if (int rc = upload(p, &p->d_blur_weights, weights.data(), weights.size())) return rc;
    if (blurs && !b.lds) MJ_HIP(q.ctx, alloc(p, &p->d_blur_scratch, (size_t)canvas + 64));
    if (hues) {
        const mj::HueTables tables = mj::colour_hue_tables();
        if (int rc = upload(p, &p->d_hue_tables, &tables, 1)) return rc;
    }
    if (out_esize > 1) {
        const std::vector<uint8_t> lut = output_table(*r.output, CO, out_esize);
        if (int rc = upload(p, &p->d_rz_lut, lut.data(), lut.size())) return rc;
        a.lut = p->d_rz_lut;
    }
    a.canvas[0] = p->d_canvas; a.canvas[1] = p->d_canvas + canvas;
    a.hist = p->d_co_hist; a.tables = p->d_co_tables; a.outputs = p->d_co_outputs; a.hist_list = p->d_co_list;
    b.list = p->d_co_list; b.weights = p->d_blur_weights; b.scratch = p->d_blur_scratch;
    h.list = p->d_co_list; h.tables = p->d_hue_tables;
    a.n_outputs = n; a.ow = r.out_width; a.oh = r.out_height; a.C = CO; a.layout = p->layout; a.esize = out_esize;
    p->colour = true;
    return MJ_OK;
}

// ---- tap tables: one per distinct axis --------------------------------------------------------------------------------------
// Where an axis lies on a placed plan's canvas: resized to `resized` entries at offset `off`; `base` is the first source entry of
// the part of the source that was decoded, `len` that part's entries.
struct AxisPlace { int resized, off, base, len; };

// Owns the tables of a plan (xs, ys: the AxisHost records the tile search reads), their serialised form for the kernels (words: per
// table ksize, first source index [out], tap count [out], taps [out][ksize]), the maps that make equal axes share a table, and the
// range check.
struct TapTables {
    const int filter;
    const bool placed, sgn;
    std::map<int, AxisHost> xs, ys;
    std::vector<int32_t> words;
    // What the kernels' arithmetic holds (resize.hip: Tap): a 24-bit multiply and a 32-bit sum — signed for the filters with side
    // lobes.  Measured over sizes 1..129 the taps stay far inside (tests/test_resample_host.py); that is no proof for every
    // size, so every table is checked and one that breaks a bound is recorded here (its sizes; 0: none) for the caller to refuse.
    int range_in = 0, range_out = 0;

    TapTables(int filter_, bool placed_) : filter(filter_), placed(placed_), sgn(mj::resize_filter_signed(filter_)) {}

    // The table of one axis in_size -> out_size, built once per distinct key.
    // back: the table of an axis the orientation reverses — entry j is entry out_size - 1 - j of the plain table read from the
    // other end of the source, taps in reverse; the sums are integer sums of the same products, and the first source index
    // still grows with j, which is what the kernels' tile bounds assume.  The kernel stores entry j at out_size - 1 - j.
    // at (placed plans, else NULL): canvas entry j is entry j - off of the table in_size -> resized, whose first source indices are
    // then counted from `base`.  A canvas entry outside the image has NO taps, and as first index the bound of the nearest entry
    // inside: the bounds still grow with j, so the kernels' tile spans hold, and a count of 0 on either axis marks a fill element —
    // an entry inside has at least one tap.  The canvas table is built first and reversed after.  Tables are then per (source
    // size, resized size, offset, reversed).
    // box (reducing plans, every axis of them; else NULL): the part of the in_size entries the table resamples, two 32-bit floats
    // (build_resize_axis) — tables are then per box as well.
    const AxisHost &axis(bool is_x, int in_size, int out_size, bool back, const AxisPlace *at, const float *box = nullptr) {
        std::map<int, AxisHost> &m = is_x ? xs : ys;
        int key = 2 * in_size + (back ? 1 : 0);
        if (placed || box) {
            std::vector<int> full{is_x, in_size, back};
            if (placed) full.insert(full.end(), {at->resized, at->off, at->base, at->len});
            if (box) { int32_t w[2]; memcpy(w, box, 8); full.insert(full.end(), {w[0], w[1]}); }
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
        if (placed) {
            const int resized = at->resized, off = at->off, base = at->base;
            A.ks = mj::resize_axis_ksize(in_size, resized, filter, box);
            std::vector<int32_t> lo((size_t)resized), cnt((size_t)resized), kk((size_t)resized * A.ks);
            mj::build_resize_axis(in_size, resized, lo.data(), cnt.data(), kk.data(), A.ks, filter, box);
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
            in_size = at->len;      // (what the reversal below counts from: the decoded part's other end)
        } else {
            A.ks = mj::resize_axis_ksize(in_size, out_size, filter, box);
            k.resize((size_t)out_size * A.ks);
            mj::build_resize_axis(in_size, out_size, A.lo.data(), A.cnt.data(), k.data(), A.ks, filter, box);
        }
        for (int j = 0; j < out_size && !range_in; ++j) {
            int64_t sum = 0, big = 0, least = 0;
            for (int t = 0; t < A.ks; ++t) {
                const int64_t v = k[(size_t)j * A.ks + t], mag = v < 0 ? -v : v;
                sum += mag; big = std::max(big, mag); least = std::min(least, v);
            }
            const int64_t top = ((int64_t)1 << 21) + 255 * sum;
            if (sgn ? (big >= (1 << 23) || top > INT32_MAX) : (least < 0 || big >= (1 << 24) || top > (int64_t)UINT32_MAX)) { range_in = A.in_size; range_out = placed ? at->resized : out_size; }
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
    }

private:
    std::map<std::vector<int>, int> placed_ids;
};

// ---- the tile ----------------------------------------------------------------------------------------------------------------
// A tile of tr rows x tc columns: what it takes in LDS and where the parts lie (ok false: it does not fit)
struct Lds { bool ok; int tr, tc, t_pitch, tab_off, stage_off, stage_bytes, lut_off, total; };
// How the plan's kernels use LDS.  xmajor: how the source is read, which for transposing orientations is the other layout's way
// (launch_resize); C: the source's components; CT: those of both passes and of T; converts: a plan of k_resize_*_mode; lut_bytes:
// the output table of a 2- or 4-byte element.
struct TileUse { bool xmajor; int C, CT; bool converts; int lut_bytes; };

// The tile: what a workgroup's LDS holds (resize.hip's kernels) must fit 64 KB — the intermediate rows of the tile, the tile's tap
// tables, the staging rows, the output table of a 2- or 4-byte element — for every source size of the batch.
Lds lds_for(const TapTables &tabs, const TileUse &u, int tr, int tc) {
    const int budget = 64 * 1024;
    int sy = 0, sx = 0, ksx = 0, ksy = 0, pitch;
    for (auto &kv : tabs.ys) { sy = std::max(sy, kv.second.span(tr)); ksy = std::max(ksy, kv.second.ks); }
    for (auto &kv : tabs.xs) { sx = std::max(sx, kv.second.span(tc)); ksx = std::max(ksx, kv.second.ks); }
    int64_t t_bytes, tab_bytes, stage = 0;
    if (u.xmajor) {
        pitch = round16((int64_t)sy * u.CT);
        t_bytes = (int64_t)tc * pitch;
        tab_bytes = ((int64_t)2 * tr + (int64_t)tr * ksy) * 4;
    } else {
        pitch = round16((int64_t)tc * u.CT);
        t_bytes = (int64_t)sy * pitch;
        tab_bytes = ((int64_t)2 * tc + (int64_t)tc * ksx) * 4;
        // (colour to L: three quarters for the staged colour row — 3 * (sx + 16) >= 3 * sx + 32 —, one for its L bytes)
        stage = u.converts && u.C == 3 ? 4 * (int64_t)round16((int64_t)sx + 16) : round16((int64_t)sx * u.C + 32);
    }
    // (grey to RGB: the tile of finished bytes behind the output table)
    const int64_t lut_off = t_bytes + round16(tab_bytes) + 4 * stage, total = lut_off + u.lut_bytes + (u.converts && u.C == 1 ? (int64_t)tr * tc : 0);
    if (total > budget) return Lds{false, tr, tc, 0, 0, 0, 0, 0, 0};
    return Lds{true, tr, tc, pitch, (int)t_bytes, (int)(t_bytes + round16(tab_bytes)), (int)stage, (int)lut_off, (int)total};
}

// A pure function of the tables, the use and the sizes (n images of out_width x out_height).  Tiles shrink until they fit: a
// row-major plan gives up columns first while a row segment stays 2 KB long (its loads run along the rows), then rows; an x-major
// plan keeps its rows (its loads run along the columns) and gives up columns.  ok false: not even a 1 x 1 tile fits.
Lds choose_tile(const TapTables &tabs, const TileUse &u, int n, int out_width, int out_height) {
    int tr = std::min<int>(u.xmajor ? 32 : 16, out_height), tc = out_width;
    auto fits = [&](int tr_, int tc_) { return lds_for(tabs, u, tr_, tc_).ok; };
    auto seg_bytes = [&](int tc_) { int sx = 0; for (auto &kv : tabs.xs) sx = std::max(sx, kv.second.span(tc_)); return sx * u.C; };
    while (!fits(tr, tc)) {
        const bool cols_first = u.xmajor ? (tc >= 32 || tr == 1) : (seg_bytes(tc) >= 2048 || tr == 1);
        if (tc > 1 && cols_first) tc = (tc + 1) / 2;
        else if (tr > 1) tr = (tr + 1) / 2;
        else return lds_for(tabs, u, 1, 1);
    }
    // (a small batch: more, smaller tiles, so that the chip has something to do)
    auto n_tiles = [&](int tr_, int tc_) { return (int64_t)n * ((out_height + tr_ - 1) / tr_) * ((out_width + tc_ - 1) / tc_); };
    while (n_tiles(tr, tc) < 1024 && tr > 4 && fits((tr + 1) / 2, tc)) tr = (tr + 1) / 2;
    return lds_for(tabs, u, tr, tc);
}

// ---- the output table, [CO][256] elements of esize bytes: the host's arithmetic, which the kernels only look up ----------------
std::vector<uint8_t> output_table(const mj_output_desc &o, int CO, int esize) {
    const bool norm = o.normalize != 0;
    std::vector<uint8_t> lut((size_t)256 * CO * esize);
    for (int c = 0; c < CO; ++c) {
        uint32_t bits[256];
        mj::build_normalize_table(o.dtype, norm ? o.mean[c] : 0.0f, norm ? o.std[c] : 1.0f, bits);
        for (int v = 0; v < 256; ++v) {
            if (esize == 4) memcpy(&lut[((size_t)c * 256 + v) * 4], &bits[v], 4);
            else { const uint16_t h = (uint16_t)bits[v]; memcpy(&lut[((size_t)c * 256 + v) * 2], &h, 2); }
        }
    }
    return lut;
}

}  // namespace

bool mj::reduce_applies(const mj_batch *b, const mj_plan_request &r) {
    if (!b || !b->images || r.reducing_gap == 0) return false;
    const mj_view *views = r.views;
    const int n_out = views ? r.n_views : b->n_images;
    for (int k = 0; k < n_out; ++k) {
        const int i = views ? views[k].image : k;
        int w = b->images[i].width, h = b->images[i].height;
        if (r.orientations && (mj::orient_bits(r.orientations[i]) & 4)) std::swap(w, h);
        if (r.rois) { w = r.rois[i].width; h = r.rois[i].height; }
        mj_roi shown, stored;
        if (views && mj::view_window(b, r.orientations, views[k], &shown, &stored)) { w = shown.width; h = shown.height; }
        const int tw = r.places ? r.places[k].width : r.out_width, th = r.places ? r.places[k].height : r.out_height;
        if (w < 1 || h < 1 || tw < 1 || th < 1) continue;
        int fx, fy;
        mj::reduce_factors(w, h, tw, th, r.reducing_gap, &fx, &fy);
        if (fx > 1 || fy > 1) return true;
    }
    return false;
}

// ---- the plan, from a normalised request with a size ------------------------------------------------------------------------------
namespace {

// What a sized request says before there is a plan: a placed request's source ranges (and the windows derived from them), whether its
// orientations exchange width and height, and its windows as windows of the stored images (rois: what the decoding plan is given).
struct Front {
    std::vector<Need> need;
    std::vector<mj_roi> derived, stored;
    const mj_roi *rois = nullptr;
    bool swapped = false;
};

int resized_front(const PlanRequest &q, bool may_window, Front &f) {
    const char *fn = mj::kCreateFn;
    mj_context *ctx = q.ctx; const mj_batch *b = q.b;
    const uint8_t *orient = q.r.orientations;
    f.rois = q.r.rois;
    if (q.r.places) {
        if (int rc = placed_source_ranges(q, may_window, f.need, f.derived)) return rc;
        if (!f.derived.empty()) f.rois = f.derived.data();
    }
    // oriented plans: all images transposing (orientations 5..8) or none — the two read their source in different ways, so
    // they are two launches, i.e. two plans (BatchDecoder sorts the files); windows are given in oriented coordinates
    if (orient) {
        if (!b->images) return fail(ctx, MJ_ERR_INVALID, "%s: NULL argument", fn);
        f.swapped = b->n_images > 0 && (mj::orient_bits(orient[0]) & 4);
        for (int i = 0; i < b->n_images; ++i)
            if (((mj::orient_bits(orient[i]) & 4) != 0) != f.swapped)
                return fail(ctx, MJ_ERR_UNSUPPORTED, "%s: image %d: orientations that exchange width and height (5..8) and others do not share a resized plan; split the batch", fn, i);
        if (f.rois) {
            if (int rc = stored_windows(q, f.rois, f.stored)) return rc;
            f.rois = f.stored.data();
        }
    }
    return MJ_OK;
}

// The stages behind the decode, built on plan p: a plan of plan_create_common's (given_src NULL: it gets its own intermediate buffer)
// or the shell of a derived plan, whose images are its parent's and whose source is the parent's buffer of given_bytes bytes.
int resized_stages(const PlanRequest &q, Front &f, mj_plan *p, uint8_t *given_src, int64_t given_bytes) {
    const char *fn = mj::kCreateFn;
    mj_context *ctx = q.ctx; const mj_batch *b = q.b;
    auto [rois_, orient, mode, out_width, out_height, transform_filter, matrices, perspective, slots, n_slots, n_views, views, output, filter,
          reducing_gap, places, fill, chains, transform_fill] = q.r;
    (void)rois_; (void)transform_filter; (void)transform_fill;
    std::vector<Need> &need = f.need;
    bool swapped = f.swapped;
    const bool affine = matrices || perspective;      // (either transform: the launch in front of the resize)
    // a plan with colour operations: the resize launch is that of the uint8, unmirrored, identity-slot request — it writes the
    // canvases —, and the element type, the slots and the mirror flags are the colour launches' (colour_stage)
    const bool colour = chains != nullptr;
    const int dtype = output ? output->dtype : MJ_DTYPE_U8, out_esize = dtype_size(dtype), esize = colour ? 1 : out_esize;
    // C: the source's components.  A plan that converts stores CO of them per pixel and runs both passes, and T, on CT = 1:
    // colour becomes L where it is read, grey becomes RGB where it is stored (resize.hip's k_resize_*_mode)
    int C = p->ncomp;
    // n: the launches' records — one per image, or one per view
    const int n = views ? n_views : p->n_images, CO = mode ? mode : C;
    int CT = mode ? 1 : C;
    p->n_views = views ? n_views : 0;
    if (mode) p->out_ncomp = CO;
    // a reducing plan (normalise_request: some image of it has a factor above 1): the resize reads the reduced images.  Colour to
    // L is then the reduce launch's — the conversion comes before the reduce — and the resize is the plain one-component one
    const bool reducing = reducing_gap != 0, luma = reducing && mode == MJ_MODE_L && C == 3;
    std::vector<Reduced> red;
    int64_t red_bytes = 0;
    if (reducing) {
        if (int rc = reduce_stage(q, p, swapped, luma, red, &red_bytes)) return rc;
        if (luma) { mode = 0; C = 1; }
    }
    // a plan with an affine transform: the resize reads upright windows of the transformed images, in the output's components —
    // mode and orientation are the affine launch's, and the resize is the plain one of CO components
    std::vector<int64_t> af_off;
    int64_t af_bytes = 0;
    if (affine) {
        if (int rc = affine_stage(q, p, CO, af_off, &af_bytes)) return rc;
        mode = 0; C = CT = CO; orient = nullptr; swapped = false;
    }
    const int64_t out_image = (int64_t)out_width * out_height * CO * esize;      // bytes
    TapTables tabs(filter, places != nullptr);
    std::vector<mj::DevResizeImage> ri((size_t)n);
    std::vector<uint8_t> flags((size_t)n, 0);      // mirror, per image
    int any_mirror = 0;
    for (int i = 0; i < n; ++i) {
        const int img = views ? views[i].image : i;
        int w = p->windowed ? p->h_win[img].w : p->h_images[img].width, h = p->windowed ? p->h_win[img].h : p->h_images[img].height;
        const int bits = orient ? mj::orient_bits(orient[img]) : 0;
        if (bits & 4) std::swap(w, h);      // (from here on the oriented image's size)
        ri[i].src_off = p->h_images[img].rgb_off;
        const int64_t slot_off = (int64_t)(slots ? slots[i] : i) * out_image;
        ri[i].dst_off = colour ? (int64_t)i * out_image : slot_off;      // (canvas i of the plan's own buffer)
        p->h_slot.push_back(slots ? slots[i] : i);      // (what mj_plan_set_erase addresses an output by)
        if (p->out_ncomp && !views) p->h_out_off.push_back(colour ? slot_off * out_esize : slot_off);
        // the record's size is what the kernels step from row to row by (resize.hip): the decoded image's.  w, h from here on: what
        // the tables are made for — the same, but for a view, whose record starts at its window's origin and whose tables are its window's
        ri[i].w = w; ri[i].h = h;
        if (views) {
            mj_roi shown, stored;
            mj::view_window(b, q.r.orientations, views[i], &shown, &stored);      // (checked by the request's normalisation)
            ri[i].src_off += pixel_offset(p->layout, p->h_images[img].width, p->h_images[img].height, p->ncomp, stored.x, stored.y);
            w = shown.width; h = shown.height;
            p->h_view_size.push_back({stored.width, stored.height});
            // (behind an affine launch: the window itself, upright and dense, in the buffer of transformed windows)
            if (affine) { ri[i].src_off = af_off[(size_t)i]; ri[i].w = w; ri[i].h = h; }
        }
        const float *bx = nullptr, *by = nullptr;
        if (reducing) {
            const Reduced &r = red[(size_t)i];
            w = r.w; h = r.h; bx = r.bx; by = r.by;
            ri[i].src_off = r.off;
            ri[i].w = w; ri[i].h = h;
            if (places) need[(size_t)i] = Need{0, w, 0, h, w, h};
        }
        if (!colour && output && output->mirror) any_mirror |= (flags[i] = output->mirror[i] ? 1 : 0);
        if (orient) flags[i] = (uint8_t)((flags[i] ^ (bits & 1)) | (bits & 2));      // (the mirror comes after the orientation)
        if (places) {
            // (w, h: what was decoded of the oriented image — the whole, the caller's window, or the derived range of either — or the view)
            const Need &nd = need[(size_t)i];
            const AxisPlace px{places[i].width, places[i].x, nd.x0, w}, py{places[i].height, places[i].y, nd.y0, h};
            ri[i].xtab = tabs.axis(true, nd.sw, out_width, bits & 1, &px, bx).word_off;
            ri[i].ytab = tabs.axis(false, nd.sh, out_height, bits & 2, &py, by).word_off;
        } else {
            ri[i].xtab = tabs.axis(true, w, out_width, bits & 1, nullptr, bx).word_off;
            ri[i].ytab = tabs.axis(false, h, out_height, bits & 2, nullptr, by).word_off;
        }
        if (tabs.range_in)
            return fail(ctx, MJ_ERR_UNSUPPORTED, "%s: resizing %d to %d with filter %d gives taps outside what the kernels' 24-bit products and 32-bit sums hold", fn,
                        tabs.range_in, tabs.range_out, filter);
        if (tabs.words.size() > ((size_t)1 << 28)) return fail(ctx, MJ_ERR_UNSUPPORTED, "%s: the tap tables of this batch are too large", fn);
    }
    const int lut_bytes = esize > 1 ? 256 * CO * esize : 0;
    const TileUse use{((p->layout & 1) == 0) != swapped, C, CT, mode != 0, lut_bytes};
    const Lds lds = choose_tile(tabs, use, n, out_width, out_height);
    if (!lds.ok) {
        int big_w = 0, big_h = 0;
        for (auto &kv : tabs.xs) big_w = std::max(big_w, kv.second.in_size);
        for (auto &kv : tabs.ys) big_h = std::max(big_h, kv.second.in_size);
        return fail(ctx, MJ_ERR_UNSUPPORTED, "%s: shrinking %d x %d sources to %d x %d takes more taps per pixel than a workgroup's LDS holds", fn,
                    big_w, big_h, out_width, out_height);
    }
    mj::ResizeArgs &a = p->rz = mj::ResizeArgs{};
    a.tr = lds.tr; a.tc = lds.tc;
    a.t_pitch = lds.t_pitch; a.tab_off = lds.tab_off; a.stage_off = lds.stage_off; a.stage_bytes = lds.stage_bytes; a.lds_bytes = lds.total;
    a.esize = esize; a.lut_off = lds.lut_off;
    a.tiles_x = (out_width + a.tc - 1) / a.tc; a.tiles_y = (out_height + a.tr - 1) / a.tr;
    const int64_t n_tiles = (int64_t)n * a.tiles_y * a.tiles_x;
    if (n_tiles > mj::kResizeGridX * (int64_t)65535)
        return fail(ctx, MJ_ERR_UNSUPPORTED, "%s: %lld tiles are more than one launch takes; split the batch", fn, (long long)n_tiles);
    a.n_images = n; a.ow = out_width; a.oh = out_height; a.layout = p->layout;
    if (int rc = upload(p, &p->d_rz_images, ri.data(), ri.size())) return rc;
    if (int rc = upload(p, &p->d_rz_tabs, tabs.words.data(), tabs.words.size())) return rc;
    a.orient = orient ? (swapped ? 2 : 1) : 0;
    a.sgn = tabs.sgn ? 1 : 0;
    p->rz_filter = filter;
    for (auto &kv : tabs.xs) p->rz_max_ksize = std::max(p->rz_max_ksize, kv.second.ks);
    for (auto &kv : tabs.ys) p->rz_max_ksize = std::max(p->rz_max_ksize, kv.second.ks);
    if (places) {
        p->rz_placed = 1;
        for (int c = 0; c < CO && fill; ++c) p->rz_fill |= (unsigned)fill[c] << (8 * c);       // (one byte per output component; fill NULL: zeros)
    }
    if (any_mirror || orient || mode || places) {       // (no flag set: the instances without mirror; a plan that converts: oriented-style instances only)
        if (int rc = upload(p, &p->d_rz_mirror, flags.data(), flags.size())) return rc;
        a.mirror = p->d_rz_mirror;
    }
    if (esize > 1) {
        const std::vector<uint8_t> lut = output_table(*output, CO, esize);
        if (int rc = upload(p, &p->d_rz_lut, lut.data(), lut.size())) return rc;
        a.lut = p->d_rz_lut;
    }
    // the un-resized pixels: a plan-owned buffer from the context's cache (64 bytes of slack: the kernels' 16-byte loads may
    // start before and end behind the bytes they use)
    if (given_src) { p->src_bytes = given_bytes; p->d_src = given_src; }
    else {
        p->src_bytes = p->info.rgb_bytes;
        MJ_HIP(ctx, alloc(p, &p->d_src, (size_t)p->src_bytes + 64));
    }
    a.images = p->d_rz_images; a.tabs = p->d_rz_tabs; a.src = p->d_src;
    if (reducing) {
        // the reduced images: a second plan-owned buffer with the same slack, which the resize launch reads as it would d_src
        MJ_HIP(ctx, alloc(p, &p->d_red, (size_t)red_bytes + 64));
        p->rd.src = p->d_src; p->rd.dst = p->d_red;
        a.src = p->d_red;
        p->reduces = true; p->rd_luma = luma;
    }
    if (affine) {
        // the transformed windows: a second plan-owned buffer with the same slack, which the resize launch reads as it would d_src
        MJ_HIP(ctx, alloc(p, &p->d_aff, (size_t)af_bytes + 64));
        p->af.src = p->pf.src = p->d_src; p->af.dst = p->pf.dst = p->d_aff;
        a.src = p->d_aff;
        p->affine = true; p->af_ncomp = CO; p->af_bytes = af_bytes;
    }
    if (colour)
        if (int rc = colour_stage(q, p, CO, out_esize)) return rc;
    p->info.rgb_bytes = (int64_t)n_slots * out_image * (colour ? out_esize : 1);
    p->info.total_pixels = (int64_t)n_slots * out_width * out_height;
    p->er_C = CO; p->er_dtype = dtype; p->er_slots = n_slots;
    p->resized = true;
    return MJ_OK;
}

}  // namespace

int mj::create_resized(const PlanRequest &q) {
    Front f;
    if (int rc = resized_front(q, true, f)) return rc;
    mj_plan *p = nullptr;
    // (whole images — also under views, which are windows of the DECODED images —: a plain plan, which may take the fused launch;
    // windows: a window plan)
    if (int rc = mj::plan_create_common(q.ctx, q.b, f.rois, f.rois != nullptr, &p)) return rc;
    PlanGuard guard{p};
    if (int rc = resized_stages(q, f, p, nullptr, 0)) return rc;
    guard.p = nullptr;
    *q.out = p;
    return MJ_OK;
}

// A derived plan: a shell with the parent's context, layout, images and component count — what the stage builders read of a plan —,
// an arena and the two events of its own; the stages are built on it over the parent's intermediate buffer, which the parent keeps
// for as long as this plan holds it (mj_plan_destroy).
int mj::create_derived(const PlanRequest &q, mj_plan *parent) {
    mj_context *ctx = q.ctx;
    Front f;
    if (int rc = resized_front(q, false, f)) return rc;
    mj_plan *p = new mj_plan();
    p->ctx = ctx; p->n_images = parent->n_images; p->layout = parent->layout; p->flags = parent->flags;
    p->hmax = parent->hmax; p->vmax = parent->vmax; p->ncomp = parent->ncomp; p->generic = parent->generic;
    p->max_pixels = parent->max_pixels; p->h_images = parent->h_images;
    p->derived = true;
    struct Guard { mj_plan *p; mj_context *c; ~Guard() { c->cur = nullptr; if (p) mj_plan_destroy(p); } } guard{p, ctx};
    if (!ctx->free_arenas.empty()) { p->arena = ctx->free_arenas.back(); ctx->free_arenas.pop_back(); }
    else if (hipHostMalloc((void **)&p->arena.base, (size_t)8 << 20, hipHostMallocDefault) == hipSuccess) p->arena.cap = (size_t)8 << 20;
    else { (void)hipGetLastError(); p->arena = mj_context::Arena{}; }
    p->arena.used = 0;
    ctx->cur = p->arena.base ? &p->arena : nullptr;
    if (int rc = resized_stages(q, f, p, parent->d_src, parent->src_bytes)) return rc;
    // (the uploads above went through the arena on the setup stream: the plan's first use waits for them, as a decoding plan's does)
    MJ_HIP(ctx, hipEventCreateWithFlags(&p->ready, hipEventDisableTiming));
    MJ_HIP(ctx, hipEventRecord(p->ready, ctx->setup_stream));
    MJ_HIP(ctx, hipEventCreateWithFlags(&p->done, hipEventDisableTiming));
    p->parent = parent;
    ++parent->refs;
    guard.p = nullptr;
    *q.out = p;
    return MJ_OK;
}

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

int mj_host_resize_table_boxed(int32_t filter, int32_t in_size, double in0, double in1, int32_t out_size, int32_t *xmin, int32_t *count, int32_t *taps,
                               int32_t taps_stride, int32_t *ksize_out) {
    if (!mj::resize_filter_known(filter) || in_size < 1 || out_size < 1 || in_size > 65535 || out_size > 65535) return MJ_ERR_INVALID;
    const float box[2] = {(float)in0, (float)in1};
    if (!(box[0] >= 0.0f) || !(box[1] <= (float)in_size) || !(box[1] > box[0])) return MJ_ERR_INVALID;
    const int ks = mj::resize_axis_ksize(in_size, out_size, filter, box);
    if (ksize_out) *ksize_out = ks;
    if (!xmin && !count && !taps) return MJ_OK;
    if (!xmin || !count || !taps || taps_stride < ks) return MJ_ERR_INVALID;
    mj::build_resize_axis(in_size, out_size, xmin, count, taps, taps_stride, filter, box);
    return MJ_OK;
}

int mj_host_resize_table(int32_t in_size, int32_t out_size, int32_t *xmin, int32_t *count, int32_t *taps, int32_t taps_stride, int32_t *ksize_out) {
    return mj_host_resize_table_filtered(MJ_FILTER_BILINEAR, in_size, out_size, xmin, count, taps, taps_stride, ksize_out);
}

int mj_host_normalize_table(int32_t dtype, float mean, float std, void *out) {
    if (!out || dtype == MJ_DTYPE_U8 || mj::output_fault(dtype, true, 1, &mean, &std)) return MJ_ERR_INVALID;
    uint32_t bits[256];
    mj::build_normalize_table(dtype, mean, std, bits);
    for (int v = 0; v < 256; ++v) {
        if (dtype == MJ_DTYPE_F32) static_cast<uint32_t *>(out)[v] = bits[v];
        else static_cast<uint16_t *>(out)[v] = (uint16_t)bits[v];
    }
    return MJ_OK;
}

int mj_debug_resize_shape(const mj_plan *p, int32_t out[8]) {
    if (!p || !out || !p->resized || p->orient_only) return MJ_ERR_INVALID;
    const mj::ResizeArgs &a = p->rz;
    const int32_t v[8] = {a.tr, a.tc, a.tiles_x, a.tiles_y, a.lds_bytes, p->rz_filter, a.sgn, p->rz_max_ksize};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return MJ_OK;
}

int mj_debug_reduce_shape(const mj_plan *p, int32_t image, int32_t out[7]) {
    if (!p || !out || !p->resized || p->orient_only || image < 0 || image >= (p->n_views ? p->n_views : p->n_images)) return MJ_ERR_INVALID;
    if (p->reduces) {
        for (int k = 0; k < 6; ++k) out[k] = p->h_rd[(size_t)image][(size_t)k];
        out[6] = 1;
        return MJ_OK;
    }
    int32_t w, h;
    if (p->n_views) { w = p->h_view_size[(size_t)image][0]; h = p->h_view_size[(size_t)image][1]; }
    else if (p->windowed) { w = p->h_win[image].w; h = p->h_win[image].h; }
    else { w = p->h_images[image].width; h = p->h_images[image].height; }
    const int32_t v[7] = {1, 1, 0, 0, w, h, 0};
    for (int k = 0; k < 7; ++k) out[k] = v[k];
    return MJ_OK;
}

int mj_debug_reduce_launch(const mj_plan *p, int32_t out[5]) {
    if (!p || !out || !p->resized || !p->reduces) return MJ_ERR_INVALID;
    const mj::ReduceArgs &a = p->rd;
    // (launch_reduce: colour to L reads three components, every other plan its own)
    const int32_t v[5] = {a.tile_slow, a.tile_fast, a.tiles_slow, a.tiles_fast, mj::reduce_piece(p->rd_luma ? 3 : p->ncomp)};
    for (int k = 0; k < 5; ++k) out[k] = v[k];
    return MJ_OK;
}

}  // extern "C"
