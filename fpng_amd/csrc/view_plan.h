// view_plan.h -- the host side of the views stage of the planar-family decode calls (include/fpng_amd.h: _planar_resize,
// _planar_resize_view, {planar,hwc}_views and their _color, _post, _warp, _tone, _enhance, _alpha and _resample siblings): what a call asks for
// (ViewRequest) and everything the batch keeps about its views (ViewPlan).  decode_api.cpp's stages each make one call into the
// plan: parse (per file: file_box, file_records, add_job; then close), place (carve_records, carve_scratch, place), plan
// (write_setup) and finish (enqueue).  Everything up to and including write_setup builds records in host memory and calls nothing
// of the HIP runtime; enqueue, the launches, is defined in decode_api.cpp.  DESIGN.md ("The views stage on the host") has the
// picture: direct and post views, how the records are indexed per job and per group, and the scratch layout.
#pragma once
#include "fpng_amd.h"
#include "resize.h"
#include "resize_color.h"
#include "resize_hwc.h"
#include "view_alpha.h"
#include "view_post.h"
#include "yuv_store.h"

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

namespace fpng_amd {

// which entry-point family was called: the last record array its signature takes
enum class ViewFamily { Plain, Color, Post, Warp, Tone, Enhance, Alpha, Resample };

// Everything a planar-family call may carry (NULL: not given).  crops and views without view_count: one view per file, whose
// destination is the planar file's own (the resize and resize_view calls); with view_count: file i has view_count[i] records of
// crops, views, dests or hwc (one of the two: planar or channels-last destinations) and of every stage's array that is given
struct ViewRequest {
    const fpng_amd_float_format *fmt = nullptr;
    const fpng_amd_crop *crops = nullptr;
    const fpng_amd_resize_view *views = nullptr;
    const uint32_t *view_count = nullptr;
    const fpng_amd_view_dest *dests = nullptr;
    const fpng_amd_view_dest_hwc *hwc = nullptr;
    const fpng_amd_view_color *colors = nullptr; // the stages' records, in the order of the calls' signatures
    const fpng_amd_view_post *posts = nullptr;
    const fpng_amd_view_warp *warps = nullptr;
    const fpng_amd_view_tone *tones = nullptr;
    const fpng_amd_view_enhance *enhances = nullptr;
    const fpng_amd_view_alpha *alphas = nullptr; // (its stage sits inside the resize, in front of all others)
    const fpng_amd_view_resample *resamples = nullptr; // (the last array of the signatures: the resize's own filter)
    // fpng_amd_decode_batch(_device)_yuv_views: the views' surfaces in the place of dests, and the call's format (judged: yuv_depth is its depth)
    const fpng_amd_yuv_dest *yuv = nullptr;
    const fpng_amd_yuv_store_format *yuv_fmt = nullptr;
    uint32_t yuv_depth = 0;
    ViewFamily family = ViewFamily::Plain;
};

struct Refusal { // code 0: none
    int code = 0;
    const char *why = nullptr;
    explicit operator bool() const { return code != 0; }
};

// the filter a view is resized with, as it travels in DecResize::filter: its RESAMPLE record's (kResizeNearest ..), where there is one
// with a filter, else the view's own
inline uint32_t view_filter(const fpng_amd_resize_view &z, const fpng_amd_view_resample *resample)
{
    return resample && resample->filter ? resample->filter + (kResizeNearest - FPNG_AMD_RESAMPLE_NEAREST) : z.filter;
}
static_assert(FPNG_AMD_RESAMPLE_NEAREST + 1 == kResizeNearest && FPNG_AMD_RESAMPLE_BOX + 1 == kResizeBox && FPNG_AMD_RESAMPLE_HAMMING + 1 == kResizeHamming &&
                  FPNG_AMD_RESAMPLE_LANCZOS + 1 == kResizeLanczos,
              "the kernels' RESAMPLE filters");

// the pixels of the file that the taps of view z of `crop` reach (fpng_amd_resize_view_source): per axis first(x) ..
// first(x + w - 1) + count(x + w - 1) of the crop's samples.  z has passed check_view_records() under its RESAMPLE record, if any (NEAREST:
// idx(x) .. idx(x + w - 1) + 1)
inline DecCrop view_box(const DecCrop &crop, const fpng_amd_resize_view &z, const fpng_amd_view_resample *resample = nullptr)
{
    uint32_t x0, x1, y0, y1;
    const uint32_t filter = view_filter(z, resample);
    resize_source_span(filter, crop.w, z.full_w, z.x, z.w, &x0, &x1);
    resize_source_span(filter, crop.h, z.full_h, z.y, z.h, &y0, &y1);
    return {crop.x + x0, crop.y + y0, x1 - x0, y1 - y0};
}

// the ONE box a file with these count >= 1 views decodes (fpng_amd_views_source): the bounding rectangle of their boxes.  The
// records have passed check_view_records(); the crops may leave the image, so the far edges are taken in 64 bits and the answer's
// w / h saturate (such a file is refused before its box is used).  each (or NULL): the views' own boxes, view_box() of each;
// resamples (or NULL): the views' RESAMPLE records
inline DecCrop views_box(const fpng_amd_crop *crops, const fpng_amd_resize_view *views, uint32_t count, DecCrop *each = nullptr, const fpng_amd_view_resample *resamples = nullptr)
{
    uint64_t x0 = UINT64_MAX, y0 = UINT64_MAX, x1 = 0, y1 = 0;
    for (uint32_t k = 0; k < count; k++) {
        const DecCrop c = {crops[k].x, crops[k].y, crops[k].w, crops[k].h};
        const DecCrop v = view_box({0, 0, c.w, c.h}, views[k], resamples ? resamples + k : nullptr); // (within the crop: no sum wraps)
        if (each) each[k] = {c.x + v.x, c.y + v.y, v.w, v.h};
        x0 = std::min<uint64_t>(x0, (uint64_t)c.x + v.x), x1 = std::max<uint64_t>(x1, (uint64_t)c.x + v.x + v.w);
        y0 = std::min<uint64_t>(y0, (uint64_t)c.y + v.y), y1 = std::max<uint64_t>(y1, (uint64_t)c.y + v.y + v.h);
    }
    return {(uint32_t)x0, (uint32_t)y0, (uint32_t)std::min<uint64_t>(x1 - x0, UINT32_MAX), (uint32_t)std::min<uint64_t>(y1 - y0, UINT32_MAX)};
}

// A destination's signed byte pitches, or why it is refused
struct DestPitches {
    int64_t pitch = 0, plane_pitch = 0;
    Refusal refused;
};
inline DestPitches refuse_dest(int code, const char *why) { return {0, 0, {code, why}}; }

// a planar destination of `planes` planes of dest_w x dest_h elements of `elem` bytes (a crop: its own w and h; a view: its
// window's): its pitches, its room
inline DestPitches judge_planar_dest(const uint8_t *d_pixels, int64_t row_pitch, int64_t plane_pitch_in, size_t pixels_cap, uint32_t dest_w, uint32_t dest_h, uint32_t planes,
                                     uint32_t elem)
{
    const uint64_t roww = (uint64_t)dest_w * elem; // bytes of a plane's row (float planes: w elements)
    if (roww >= 0x80000000ull) return refuse_dest(FPNG_AMD_ERR_INVALID_ARG, "w * element bytes >= 2^31");
    const int64_t pitch = row_pitch ? row_pitch : (int64_t)roww;
    const uint64_t step = (uint64_t)(pitch < 0 ? -pitch : pitch);
    if (step < roww) return refuse_dest(FPNG_AMD_ERR_INVALID_ARG, "|row_pitch| < w (* element bytes)");
    const uint64_t span = (uint64_t)(dest_h - 1) * step + roww; // a plane, from its lowest row's first byte
    const int64_t plane_pitch = plane_pitch_in ? plane_pitch_in : (int64_t)((uint64_t)dest_h * step);
    if (plane_pitch == INT64_MIN) return refuse_dest(FPNG_AMD_ERR_INVALID_ARG, "plane_pitch out of range");
    const uint64_t pstep = (uint64_t)(plane_pitch < 0 ? -plane_pitch : plane_pitch);
    if (pstep < span) return refuse_dest(FPNG_AMD_ERR_INVALID_ARG, "|plane_pitch| < (h - 1) * |row_pitch| + w (* element bytes): the planes overlap");
    if (pstep > (UINT64_MAX >> 3)) return refuse_dest(FPNG_AMD_ERR_INVALID_ARG, "plane_pitch out of range");
    if (!d_pixels || pixels_cap < (uint64_t)(planes - 1) * pstep + span)
        return refuse_dest(FPNG_AMD_ERR_BUFFER_TOO_SMALL, "d_pixels / pixels_cap < (num_chans - 1) * |plane_pitch| + (h - 1) * |row_pitch| + w (* element bytes)");
    return {pitch, plane_pitch, {}};
}

// the sibling for a channels-last destination of dest_w x dest_h pixels of pixel_elems elements, `planes` of them written: the
// rows' pitch and the room (fpng_amd_view_dest_hwc's rule; the record's own rules: check_views_request, decode_files_planar)
inline DestPitches judge_hwc_dest(const fpng_amd_view_dest_hwc &d, uint32_t dest_w, uint32_t dest_h, uint32_t planes, uint32_t elem)
{
    const uint32_t px = d.pixel_elems ? d.pixel_elems : planes;
    const uint64_t span = ((uint64_t)(dest_w - 1) * px + planes) * elem; // a row, from its first byte to its last written one
    if (span >= 0x80000000ull) return refuse_dest(FPNG_AMD_ERR_INVALID_ARG, "((w - 1) * pixel_elems + num_chans) * element bytes >= 2^31");
    const int64_t pitch = d.row_pitch ? d.row_pitch : (int64_t)((uint64_t)dest_w * px * elem);
    const uint64_t step = (uint64_t)(pitch < 0 ? -pitch : pitch);
    if (step >= 0x80000000ull) return refuse_dest(FPNG_AMD_ERR_INVALID_ARG, "w * pixel_elems * element bytes >= 2^31");
    if (step < span) return refuse_dest(FPNG_AMD_ERR_INVALID_ARG, "|row_pitch| < ((w - 1) * pixel_elems + num_chans) * element bytes");
    if (!d.d_pixels || d.pixels_cap < (uint64_t)(dest_h - 1) * step + span)
        return refuse_dest(FPNG_AMD_ERR_BUFFER_TOO_SMALL, "d_pixels / pixels_cap < (h - 1) * |row_pitch| + ((w - 1) * pixel_elems + num_chans) * element bytes");
    return {pitch, 0, {}};
}

// a YUV surface of `surface` for a view of w x h pixels (fpng_amd_yuv_dest's rules).  room: d_luma and surface_cap are judged too
// (a file whose header is accepted); pitch: the rows' pitch in bytes
inline Refusal judge_yuv_dest(const fpng_amd_yuv_dest &d, uint32_t surface, uint32_t w, uint32_t h, bool room, int64_t *pitch_out = nullptr)
{
    const int kBad = FPNG_AMD_ERR_INVALID_ARG;
    if (d.reserved) return {kBad, "fpng_amd_yuv_dest::reserved must be 0"};
    const uint64_t elem = yuv_elem_bytes(surface);
    if ((uint64_t)w * elem >= 0x80000000ull - 16) return {kBad, "w * element bytes >= 2^31 - 16"}; // (a chroma row and the scratch planes' pitch stay below 2^31)
    const int64_t row_bytes = (int64_t)((uint64_t)w * elem), chroma_bytes = (int64_t)yuv_chroma_row_bytes(surface, w);
    if (d.row_pitch < 0) return {kBad, "row_pitch must not be negative"};
    if (elem > 1 && (((uintptr_t)d.d_luma | (uint64_t)d.row_pitch | (uint64_t)d.chroma_offset) & 1u))
        return {kBad, "d_luma, row_pitch and chroma_offset must be multiples of 2 on 16-bit surfaces"};
    const int64_t pitch = d.row_pitch ? d.row_pitch : std::max(row_bytes, chroma_bytes);
    if (pitch < row_bytes) return {kBad, "row_pitch < w (* element bytes)"};
    if (pitch < chroma_bytes) return {kBad, "row_pitch < 2 * ceil(w / 2) (* element bytes): an odd width's last pixel has a full chroma pair"};
    if (pitch >= (int64_t)0x80000000ll) return {kBad, "row_pitch >= 2^31"};
    const int64_t limit = INT64_MAX >> 2; // (two offsets and a plane's span stay inside 64 bits)
    if (d.chroma_offset < -limit || d.chroma_offset > limit) return {kBad, "chroma_offset out of range"};
    const int64_t span = (int64_t)(h - 1) * pitch + row_bytes; // bytes from the luma plane's first row to the end of its last
    // (a 4:2:0 chroma plane in FRONT of the luma plane ends (h + 1) / 2 - 1 rows and a chroma row behind its start)
    const int64_t chroma_span = yuv_is_420(surface) ? (int64_t)(((uint64_t)h + 1) / 2 - 1) * pitch + chroma_bytes : span;
    const int64_t aco = d.chroma_offset < 0 ? -d.chroma_offset : d.chroma_offset;
    if (aco < span || (d.chroma_offset < 0 && aco < chroma_span)) return {kBad, "|chroma_offset| < (h - 1) * row_pitch + w (* element bytes): the planes overlap"};
    // from the lowest plane's top row to the last element of the highest one
    const uint64_t need = yuv_is_420(surface) ? (uint64_t)aco + (uint64_t)(d.chroma_offset < 0 ? span : chroma_span) : 2 * (uint64_t)aco + (uint64_t)span;
    if (room && (!d.d_luma || d.surface_cap < need)) return {FPNG_AMD_ERR_BUFFER_TOO_SMALL, "d_luma / surface_cap < the surface's bytes, from the lowest plane's top row to the last element of the highest"};
    if (pitch_out) *pitch_out = pitch;
    return {};
}

// One call's views.  A RECORD is a view of a file that became a job, numbered in the views' order over the jobs; job k's records
// are job_rec[k] .. job_rec[k + 1] - 1.  A view with a post flag, a warp that moves, a tone or an enhance op is a POST view: its
// resize record writes the un-mirrored uint8 window into the scratch and its destination travels in a DecViewPost record to
// dec_view_post_kernel; every other view is a DIRECT view, whose resize record writes the destination.  The views of a YUV call
// (rq.yuv) are direct views whose destinations the plan itself places in the scratch -- three uint8 planes, rows yuv_stage_pitch()
// apart -- and whose surfaces travel in DecYuvStore records to dec_yuv_store_kernel (yuv_store.h).  An empty plan (a call
// without views) holds nothing and every method returns at once.
struct ViewPlan {
    ViewRequest rq;      // as normalised by decode_api.cpp (normalise_views): posts only when some view is a post view, and then with colors
    uint32_t elem = 1;   // bytes of a destination element
    std::vector<uint32_t> view_ofs; // per file: its first record of the request's arrays (with view_count)

    std::vector<DecResize> resize; // per record (src, and a post view's dst: offsets into the intermediate planes until place())
    std::vector<uint32_t> tiles, lds;                  // per record: its tiles per plane, the LDS bytes of one
    std::vector<std::pair<uint32_t, uint32_t>> hwc_px; // per record of a per-tile launch: pixel_elems and flags (direct channels-last views; else 0, 0)
    std::vector<uint32_t> color_view;                  // per record of a colour launch: its view's index in rq.colors
    std::vector<int32_t> post_of;                      // per record of a post call: its index in post_recs, or -1 for a direct view
    std::vector<DecViewPost> post_recs;                // per post view
    std::vector<DecYuvStore> yuv_recs;                 // per record of a YUV call: its surface (src: an offset into the intermediate planes until place())
    std::vector<uint64_t> yuv_pre;                     // ... and one more: the workgroups of dec_yuv_store_kernel of the records in front
    std::vector<DecToneRef> tone_refs;                 // per tone view -- a post view with a tone op -- and the entry that closes the sums
    std::vector<uint32_t> job_rec, job_post, job_tone; // per job and one more: its first record, post record and tone view
    // the NEAREST views' indices (resize.h: DecResize::nearest), w + h words per such record, in the records' order; until place()
    // a record's `nearest` is 1 + the index of its first word here (NULL: not a NEAREST view)
    std::vector<uint32_t> nearest;
    // the launches' prefix sums, an entry per record and one more: workgroups (planes x tiles) of the records in front, their tiles
    // (the per-tile launches), and in a post call the tiles of the direct and of the post records, each kind counted on its own
    std::vector<uint64_t> plane_pre, tile_pre, dir_pre, post_pre;
    size_t mid_total = 0; // bytes of the intermediate planes: per job its box's, then its post views' windows, 16-byte aligned each

    std::vector<DecResize> file_recs; // (the file at hand: its views' records, their source boxes, pixel_elems and flags)
    std::vector<DecCrop> file_boxes;
    std::vector<std::pair<uint32_t, uint32_t>> file_px;
    std::vector<DecYuvStore> file_yuv;  // (a YUV call: its views' surfaces)
    std::vector<uint32_t> file_nearest; // (its NEAREST views' indices; a record's `nearest`: 1 + its first word's index here)

    // the scratch: offsets from carve_*(), pointers from place().  recs, pre, post, tone_refs lie inside the set-up block
    struct Carves {
        size_t recs = 0, pre = 0, post = 0, tone_refs = 0, nearest = 0, yuv = 0, yuv_pre = 0, mid = 0, tone = 0;
    } at;
    uint8_t *d_recs = nullptr, *d_mid = nullptr, *d_tone = nullptr;
    uint64_t *d_pre = nullptr;
    uint32_t *d_nearest = nullptr;
    DecViewPost *d_post = nullptr;
    DecToneRef *d_tone_refs = nullptr;
    DecYuvStore *d_yuv = nullptr;
    uint64_t *d_yuv_pre = nullptr;

    bool active() const { return rq.views != nullptr; }
    bool multi() const { return rq.view_count != nullptr; }
    bool hwc() const { return rq.hwc != nullptr; }
    bool per_tile() const { return rq.hwc || rq.colors; } // a workgroup per (record, tile), all planes: dec_resize_hwc_kernel, dec_resize_color_kernel
    size_t rec_bytes() const { return rq.colors ? sizeof(DecResizeColor) : rq.hwc ? sizeof(DecResizeHwc) : sizeof(DecResize); }
    size_t n_tone() const { return tone_refs.empty() ? 0 : tone_refs.size() - 1; }
    uint32_t first_view(uint32_t file) const { return multi() ? view_ofs[file] : file; }
    uint32_t views_of(uint32_t file) const { return multi() ? rq.view_count[file] : 1u; }

    // the alpha op and background of view `view` as they travel in DecResize::flags.  file_chans: the channels of the view's FILE --
    // a file without an alpha plane has P_3 = 255, for which every op is the identity: its records normalise to op 0
    uint32_t filter_of(uint32_t view) const { return view_filter(rq.views[view], rq.resamples ? rq.resamples + view : nullptr); }

    uint32_t alpha_flags(uint32_t view, uint32_t file_chans) const { return rq.alphas && file_chans == 4 ? resize_alpha_flags(rq.alphas[view]) : 0u; }

    // the planes that file i's job decodes into the scratch: the destination's `planes`, and all four of a 4-channel file of which
    // some view has an alpha op -- its fourth plane is read even where the destination has three
    uint32_t job_planes(uint32_t i, uint32_t file_chans, uint32_t planes) const
    {
        for (uint32_t v = first_view(i), end = v + views_of(i); v < end; v++)
            if (alpha_flags(v, file_chans)) return 4;
        return planes;
    }

    // ---- parse ----
    void begin(const ViewRequest &request, uint32_t n_files, uint32_t elem_bytes)
    {
        rq = request, elem = elem_bytes;
        if (multi()) { // (the counts' sum fits 32 bits: check_views_request)
            view_ofs.resize(n_files);
            for (uint32_t i = 0, at_view = 0; i < n_files; at_view += rq.view_count[i++]) view_ofs[i] = at_view;
        }
        if (active()) plane_pre.assign(1, 0), tile_pre.assign(1, 0);
        if (rq.yuv) yuv_pre.assign(1, 0);
    }

    // what the crop stage decodes of file i: the ONE box that holds the boxes of all of its views (which file_records() uses)
    DecCrop file_box(uint32_t i)
    {
        const uint32_t v0 = first_view(i), nv = views_of(i);
        file_boxes.resize(nv);
        return views_box(rq.crops + v0, rq.views + v0, nv, file_boxes.data(), rq.resamples ? rq.resamples + v0 : nullptr);
    }

    // the destinations of file i's views judged, and a record per view for the resize kernels, which read the view's own box inside
    // the planes of the job's box `crop` (src: an offset from those planes' first byte until the file is known to become a job).
    // f, x: the file, whose own destination is the view's in the calls with one view per file; planes: its num_chans; file_chans:
    // the channels in the file (alpha_flags)
    Refusal file_records(uint32_t i, const fpng_amd_png &f, const fpng_amd_png_planar &x, uint32_t planes, const DecCrop &crop, uint32_t file_chans = 0)
    {
        if (crop.w >= 0x80000000u) return {FPNG_AMD_ERR_INVALID_ARG, "crop.w >= 2^31"};
        const uint32_t v0 = first_view(i), nv = views_of(i);
        file_recs.clear(), file_px.clear(), file_nearest.clear(), file_yuv.clear();
        for (uint32_t v = v0; v < v0 + nv; v++) {
            const fpng_amd_resize_view &z = rq.views[v];
            fpng_amd_view_dest dest = rq.hwc     ? fpng_amd_view_dest{rq.hwc[v].d_pixels, 0, 0, 0}
                                      : rq.dests ? rq.dests[v]
                                                 : fpng_amd_view_dest{(uint8_t *)f.d_pixels, x.row_pitch, x.plane_pitch, f.pixels_cap};
            DestPitches d;
            if (rq.yuv) { // (the resize writes three uint8 planes into the scratch, as a post view's; the surface travels to dec_yuv_store_kernel)
                int64_t pitch = 0;
                if (const Refusal no = judge_yuv_dest(rq.yuv[v], rq.yuv_fmt->surface, z.w, z.h, true, &pitch)) return no;
                const uint32_t stage = yuv_stage_pitch(z.w);
                file_yuv.push_back({nullptr, (uint8_t *)rq.yuv[v].d_luma, pitch, rq.yuv[v].chroma_offset, (uint64_t)stage * z.h, stage, z.w, z.h, 0});
                dest.d_pixels = nullptr, d.pitch = (int64_t)stage, d.plane_pitch = (int64_t)((uint64_t)stage * z.h);
            } else
                d = rq.hwc ? judge_hwc_dest(rq.hwc[v], z.w, z.h, planes, elem) : judge_planar_dest(dest.d_pixels, dest.row_pitch, dest.plane_pitch, dest.pixels_cap, z.w, z.h, planes, elem);
            if (d.refused) return d.refused;
            if (resize_tiles(z.w, z.h) * 4 * kResizeBlock >= (1ull << 32)) return {FPNG_AMD_ERR_UNSUPPORTED, "an output size of more than 2^22 tiles of 64 x 16"};
            const DecCrop whole_crop = {rq.crops[v].x, rq.crops[v].y, rq.crops[v].w, rq.crops[v].h}, box = file_boxes[v - v0];
            DecResize rs = {};
            rs.src = (const uint8_t *)(uintptr_t)((size_t)(box.y - crop.y) * crop.w + (box.x - crop.x));
            rs.src_pitch = crop.w, rs.src_plane_pitch = (uint64_t)crop.w * crop.h;
            rs.dst = dest.d_pixels, rs.plane_pitch = d.plane_pitch, rs.pitch = (int32_t)d.pitch;
            rs.in_w = whole_crop.w, rs.in_h = whole_crop.h, rs.full_w = z.full_w, rs.full_h = z.full_h, rs.flags = z.flags | alpha_flags(v, file_chans), rs.planes = planes, rs.filter = filter_of(v);
            rs.x = z.x, rs.y = z.y, rs.w = z.w, rs.h = z.h;
            rs.box_x = box.x - whole_crop.x, rs.box_y = box.y - whole_crop.y;
            rs.taps_x = resize_max_taps(rs.in_w, z.full_w, rs.filter), rs.taps_y = resize_max_taps(rs.in_h, z.full_h, rs.filter), rs.rows = resize_tile_rows(rs.in_h, z.full_h, rs.filter);
            if (rs.filter == kResizeNearest) { // (the window's columns, then its rows, as samples of the crop)
                const size_t at = file_nearest.size();
                file_nearest.resize(at + (size_t)z.w + z.h);
                if (!resize_nearest_indices(rs.in_w, z.full_w, z.x, z.w, file_nearest.data() + at) || !resize_nearest_indices(rs.in_h, z.full_h, z.y, z.h, file_nearest.data() + at + z.w))
                    return {FPNG_AMD_ERR_UNSUPPORTED, "a NEAREST index outside the crop"};
                rs.nearest = (const uint32_t *)(uintptr_t)(at + 1);
            }
            file_recs.push_back(rs);
            if (rq.hwc) file_px.push_back({rq.hwc[v].pixel_elems ? rq.hwc[v].pixel_elems : planes, rq.hwc[v].flags});
        }
        return {};
    }

    bool is_post_view(uint32_t view) const
    {
        return rq.posts && (rq.posts[view].flags || (rq.warps && warp_moves(rq.warps[view])) || (rq.tones && rq.tones[view].op) || (rq.enhances && rq.enhances[view].op));
    }

    // file i becomes the next job: its records of file_records() join the plan.  The crop kernels write tight uint8 planes of the
    // box's size into the scratch; the resize reads them and writes the caller's.  Returns the planes' offset (the job's `out`
    // until place()); their pitches are crop.w and crop.w * crop.h.  in_scratch: job_planes() of the file (0: `planes`)
    size_t add_job(uint32_t i, uint32_t planes, const DecCrop &crop, uint32_t in_scratch = 0)
    {
        const uint32_t v0 = first_view(i);
        job_rec.push_back((uint32_t)resize.size());
        job_tone.push_back((uint32_t)tone_refs.size());
        for (DecResize &rs : file_recs) {
            rs.src += mid_total; // (an offset until place())
            if (rs.nearest) rs.nearest = (const uint32_t *)((uintptr_t)rs.nearest + nearest.size()); // (1 + an index until place())
            const uint64_t n_tiles = resize_tiles(rs.w, rs.h);
            const uint32_t k = (uint32_t)(&rs - file_recs.data()), view = v0 + k;
            const bool is_post = is_post_view(view);
            if (is_post) { // (the destination goes to the post stage; the resize writes tight un-mirrored uint8 planes)
                const fpng_amd_view_post &vp = rq.posts[view];
                DecViewPost pr = {};
                pr.dst = rs.dst, pr.plane_pitch = rs.plane_pitch, pr.pitch = rs.pitch, pr.w = rs.w, pr.h = rs.h, pr.planes = rs.planes, pr.mirror = rs.flags & kResizeMirror;
                if (rq.hwc) pr.pixel_elems = file_px[k].first, pr.hwc_flags = file_px[k].second;
                pr.flags = vp.flags, pr.radius = vp.blur_radius, pr.threshold = vp.solarize_threshold, pr.bits = vp.posterize_bits;
                if (vp.flags & kPostBlur) post_blur_weights(vp.blur_radius, vp.blur_sigma, pr.k);
                if (rq.warps) pr.warp = warp_record(rq.warps[view]);
                if (rq.enhances) pr.enhance_op = rq.enhances[view].op, pr.enhance_factor = rq.enhances[view].factor;
                if (rq.tones && rq.tones[view].op) { // (tone: an offset until place())
                    pr.tone_op = rq.tones[view].op, pr.tone_factor = rq.tones[view].factor;
                    tone_refs.push_back({tone_chunks_so_far(), (uint32_t)post_recs.size(), 0});
                }
                post_recs.push_back(pr);
                rs.dst = nullptr, rs.pitch = (int32_t)rs.w, rs.plane_pitch = (int64_t)((uint64_t)rs.w * rs.h), rs.flags &= ~kResizeMirror;
            }
            if (rq.posts) post_of.push_back(is_post ? (int32_t)post_recs.size() - 1 : -1);
            resize.push_back(rs);
            tiles.push_back((uint32_t)n_tiles), lds.push_back(resize_tile_lds(rs.taps_x, rs.taps_y, rs.rows));
            plane_pre.push_back(plane_pre.back() + rs.planes * n_tiles);
            if (per_tile()) { // (a workgroup per tile, all planes; channels-last: the tile's result bytes in its LDS)
                if (rq.hwc && !is_post) lds.back() = resize_hwc_tile_lds(rs.taps_x, rs.taps_y, rs.rows, rs.planes);
                tile_pre.push_back(tile_pre.back() + n_tiles);
                hwc_px.push_back(rq.hwc && !is_post ? file_px[k] : std::pair<uint32_t, uint32_t>{0, 0});
                if (rq.colors) color_view.push_back(view);
            }
        }
        nearest.insert(nearest.end(), file_nearest.begin(), file_nearest.end());
        const size_t out = mid_total;
        mid_total += ((size_t)crop.w * crop.h * (in_scratch ? in_scratch : planes) + 15) & ~(size_t)15;
        // (a YUV call's views: their three planes next to the box's, rows and planes a multiple of 16 bytes)
        for (size_t q = job_rec.back(), k = 0; rq.yuv && q < resize.size(); q++, k++) {
            resize[q].dst = (uint8_t *)(uintptr_t)mid_total; // (an offset until place())
            yuv_recs.push_back(file_yuv[k]);
            yuv_pre.push_back(yuv_pre.back() + yuv_store_blocks(rq.yuv_fmt->surface, resize[q].w, resize[q].h));
            mid_total += (size_t)yuv_recs.back().src_plane_pitch * 3;
        }
        // (the post views' windows: next to the box's planes)
        for (size_t q = job_rec.back(); rq.posts && q < resize.size(); q++)
            if (post_of[q] >= 0) {
                resize[q].dst = (uint8_t *)(uintptr_t)mid_total; // (an offset until place())
                mid_total += ((size_t)resize[q].w * resize[q].h * planes + 15) & ~(size_t)15;
            }
        return out;
    }

    // the chunks of dec_view_tone_hist_kernel of the tone views so far
    uint64_t tone_chunks_so_far() const
    {
        if (tone_refs.empty()) return 0;
        const DecViewPost &last = post_recs[tone_refs.back().rec];
        return tone_refs.back().pre + tone_chunks(last.w, last.h);
    }

    // behind the last file: the entries that close the per-job indices and the tone views' sums
    void close()
    {
        if (!active()) return;
        job_rec.push_back((uint32_t)resize.size());
        job_tone.push_back((uint32_t)tone_refs.size());
        if (!tone_refs.empty()) tone_refs.push_back({tone_chunks_so_far(), 0, 0});
    }

    // ---- place: sc.carve(bytes) hands out the next piece of the scratch.  The records, the prefix sums, the post records and the
    //      tone refs are carved inside the set-up block; the intermediate planes and the tone views' histograms and tables, which
    //      are written on the device, behind it ----
    template <class S> void carve_records(S &sc)
    {
        at.recs = sc.carve(resize.size() * rec_bytes());
        at.pre = sc.carve(multi() ? (plane_pre.size() + (rq.posts ? 1 : 0)) * sizeof(uint64_t) : 0);
        at.post = sc.carve(post_recs.size() * sizeof(DecViewPost));
        at.tone_refs = sc.carve(tone_refs.size() * sizeof(DecToneRef));
        at.nearest = sc.carve(nearest.size() * sizeof(uint32_t));
        at.yuv = sc.carve(yuv_recs.size() * sizeof(DecYuvStore));
        at.yuv_pre = sc.carve(yuv_pre.size() * sizeof(uint64_t));
    }
    template <class S> void carve_scratch(S &sc)
    {
        at.mid = active() ? sc.carve(mid_total) : 0; // (the crops' uint8 planes between the crop kernels and the resize)
        at.tone = sc.carve(n_tone() * kToneBytes);
    }
    // the offsets become pointers (a job's `out`: d_mid + its offset, the caller's to patch)
    void place(uint8_t *base)
    {
        if (!active()) return;
        d_recs = base + at.recs, d_mid = base + at.mid;
        d_pre = multi() ? (uint64_t *)(base + at.pre) : nullptr;
        d_nearest = (uint32_t *)(base + at.nearest);
        d_yuv = rq.yuv ? (DecYuvStore *)(base + at.yuv) : nullptr, d_yuv_pre = rq.yuv ? (uint64_t *)(base + at.yuv_pre) : nullptr;
        d_post = rq.posts ? (DecViewPost *)(base + at.post) : nullptr;
        d_tone_refs = n_tone() ? (DecToneRef *)(base + at.tone_refs) : nullptr, d_tone = n_tone() ? base + at.tone : nullptr;
        for (size_t t = 0; t < n_tone(); t++) post_recs[tone_refs[t].rec].tone = (uint32_t *)(d_tone + t * kToneBytes);
        for (size_t q = 0; q < resize.size(); q++) {
            resize[q].src = d_mid + (size_t)(uintptr_t)resize[q].src;
            if (resize[q].nearest) resize[q].nearest = d_nearest + ((size_t)(uintptr_t)resize[q].nearest - 1);
            if (rq.posts && post_of[q] >= 0) post_recs[post_of[q]].src = resize[q].dst = d_mid + (size_t)(uintptr_t)resize[q].dst;
            if (rq.yuv) yuv_recs[q].src = resize[q].dst = d_mid + (size_t)(uintptr_t)resize[q].dst;
        }
    }

    // ---- plan ----
    // record q as its launch's kernel reads it, into rec_bytes() zeroed bytes: DecResize, which DecResizeHwc (pixel_elems, flags)
    // and then DecResizeColor (the matrix) extend at the back, without padding
    void put_record(uint8_t *to, size_t q) const
    {
        std::memcpy(to, &resize[q], sizeof(DecResize));
        if (per_tile()) {
            const uint32_t px[2] = {hwc_px[q].first, hwc_px[q].second};
            std::memcpy(to + offsetof(DecResizeHwc, pixel_elems), px, sizeof px);
        }
        if (rq.colors) std::memcpy(to + offsetof(DecResizeColor, m), rq.colors[color_view[q]].m, sizeof(DecResizeColor::m));
    }
    static_assert(sizeof(DecResizeHwc) == sizeof(DecResize) + 8 && offsetof(DecResizeHwc, hwc_flags) == offsetof(DecResizeHwc, pixel_elems) + 4 &&
                      sizeof(DecResizeColor) == sizeof(DecResizeHwc) + sizeof(DecResizeColor::m),
                  "the resize records extend each other without padding");

    // the records and their prefix sums into the host copy of the set-up block (whose first byte is byte `setup_ofs` of the
    // scratch).  A post call's records go up as two arrays, the direct ones in front, each kind in the views' order and with the
    // tiles in front of it: direct record d0 .. of job k is its record number minus job_post[k]
    void write_setup(uint8_t *h_setup, size_t setup_ofs)
    {
        if (!active()) return;
        uint8_t *const h_recs = h_setup + (at.recs - setup_ofs), *const h_pre = h_setup + (at.pre - setup_ofs);
        const size_t nd = resize.size() - post_recs.size(), step = rec_bytes();
        if (!nearest.empty()) std::memcpy(h_setup + (at.nearest - setup_ofs), nearest.data(), nearest.size() * sizeof(uint32_t));
        if (!yuv_recs.empty()) {
            std::memcpy(h_setup + (at.yuv - setup_ofs), yuv_recs.data(), yuv_recs.size() * sizeof(DecYuvStore));
            std::memcpy(h_setup + (at.yuv_pre - setup_ofs), yuv_pre.data(), yuv_pre.size() * sizeof(uint64_t));
        }
        size_t di = 0, pi = 0;
        if (rq.posts) dir_pre.assign(1, 0), post_pre.assign(1, 0), job_post.clear();
        for (size_t k = 0, q = 0; k < job_rec.size(); k++) {
            for (; q < job_rec[k]; q++) {
                const bool is_post = rq.posts && post_of[q] >= 0;
                put_record(h_recs + (is_post ? nd + pi++ : di++) * step, q);
                if (rq.posts) {
                    std::vector<uint64_t> &pre = is_post ? post_pre : dir_pre;
                    pre.push_back(pre.back() + tiles[q]);
                }
            }
            if (rq.posts) job_post.push_back((uint32_t)pi);
        }
        if (rq.posts) {
            if (!post_recs.empty()) std::memcpy(h_setup + (at.post - setup_ofs), post_recs.data(), post_recs.size() * sizeof(DecViewPost));
            if (!tone_refs.empty()) std::memcpy(h_setup + (at.tone_refs - setup_ofs), tone_refs.data(), tone_refs.size() * sizeof(DecToneRef));
            std::memcpy(h_pre, dir_pre.data(), dir_pre.size() * sizeof(uint64_t));
            std::memcpy(h_pre + (nd + 1) * sizeof(uint64_t), post_pre.data(), post_pre.size() * sizeof(uint64_t));
        } else if (multi()) { // (the launch's prefix sums: planes x tiles, the channels-last and colour calls': tiles)
            const std::vector<uint64_t> &pre = per_tile() ? tile_pre : plane_pre;
            std::memcpy(h_pre, pre.data(), pre.size() * sizeof(uint64_t));
        }
    }

    // ---- finish (decode_api.cpp): the launches of the records of jobs j0 .. j1 - 1 on stream s, behind the group's pixel pass ----
    int enqueue(hipStream_t s, uint32_t j0, uint32_t j1, const DecFloat *flt) const;
};

} // namespace fpng_amd
