// view_request.h -- how a views request is judged and normalised, and the views path of the fpng tier, for the callers outside
// decode_api.cpp (png_views_api.cpp).  The bodies, and the rules' text, are decode_api.cpp's.
#pragma once
#include "view_plan.h"

#include <vector>

struct fpng_amd_encoder;

namespace fpng_amd {

// which stages some view of a request really uses
struct StagesUsed {
    bool post = false, warp = false, tone = false, enhance = false;
    uint64_t total = 0; // the views of the call, where the counts are good
};
// what normalise_views supplies, kept alive by the caller
struct ViewDefaults {
    std::vector<fpng_amd_view_post> posts;
    std::vector<fpng_amd_view_color> colors;
};

// what needs no file, no encoder and no device, in the views calls' order (rq.family names the call)
int check_views_request(const fpng_amd_png_planar *files, uint32_t n, const ViewRequest &rq, const fpng_amd_decode_result *results, StagesUsed &used);
// THE normalisation rule of the views calls
ViewRequest normalise_views(ViewRequest rq, const StagesUsed &used, ViewDefaults &made);
// The words that the planar family judges behind the encoder (decode_files_planar), for it and for the views of ordinary PNG files.
// fmt (or NULL: uint8, elem 1) -> flt, and elem, the bytes of an element
int check_float_format(const fpng_amd_float_format *fmt, DecFloat &flt, uint32_t &elem);
// every view's destination, hwc's then dests': whole elements, |row_pitch| < 2^31
int check_view_dests(const ViewRequest &rq, uint64_t n_views, uint32_t elem);
// fpng-written files through the views call of asked.family
int decode_files_views(fpng_amd_encoder *e, const fpng_amd_png_planar *files, uint32_t n, fpng_amd_decode_result *results, bool device_data, const ViewRequest &asked);

} // namespace fpng_amd
