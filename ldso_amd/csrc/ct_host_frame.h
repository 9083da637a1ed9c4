// ct_host_frame.h -- the new frame: makeImages' pyramid, frame ingestion from the raw image, and the frame's read-backs
// (k_ct_pyramid.h, k_ct_undistort.h).  Owns c->frame; every other part reads frame.d_dIp.
// A piece of the one translation unit ldso_ct.hip (k_ct_pyramid.h).
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ldso_ba_internal.h"
#include "ct_context.h"

#pragma clang fp contract(off)

// the BA frame store's view of the new frame (ldso_ba_frame_put_tracker)
int ldso_ba::ct_frame_view(const ldso_ct_ctx *c, ldso_ba::CtFrameView *out) {
    if (!c || !out) return fail(-1, "null argument");
    out->intensity = c->frame.d_inten.p;
    out->texels = c->frame.d_dIp.p;
    out->width = c->pyr.w;
    out->height = c->pyr.h;
    out->device = c->device;
    out->stream = (void *)c->stream;
    out->have_frame = c->frame.have;
    return 0;
}

namespace {

// ---- the new frame (k_ct_pyramid.h, k_ct_undistort.h) --------------------------------------------
// makeImages behind a level-0 image in d_color: the response table's upload and the two pyramid launches
// on the context's stream, no synchronisation.  Both ways of setting the new frame end here.
int frame_pyramid(ldso_ct_ctx *c, const float *b_response) {
    const PyrParams &P = c->pyr;
    if (b_response)
        HIP_TRY(hipMemcpyAsync(c->frame.d_B.p, b_response, 256 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const float *B = b_response ? c->frame.d_B.p : nullptr;
    const dim3 grid(P.w / P.tile, P.h / P.tile);
    const size_t lds = ((size_t)P.tile * P.tile + (size_t)(P.tile / 2) * (P.tile / 2) + 1) * sizeof(float);
    int rc = ct_launch(c, kCtSlotPyrDown,
                       [&] { k_ct_pyr_down<<<grid, kCtThreads, lds, c->stream>>>(c->frame.d_color.p, c->frame.d_inten.p, P); });
    if (rc) return rc;
    const int npx = P.off[P.levels];
    return ct_launch(c, kCtSlotPyrGrad, [&] {
        k_ct_pyr_grad<<<(npx + kCtThreads - 1) / kCtThreads, kCtThreads, 0, c->stream>>>(c->frame.d_inten.p, c->frame.d_dIp.p, B, P);
    });
}

// What processFrame does with this frame (Undistort.cc:198-228): the photometric value of a source pixel and
// ImageAndExposure::exposure_time.  Refuses what the frame cannot be read with.
int und_frame_mode(const ldso_ct_ctx *c, int bits, float exposure_time, int &mode, float &exposure) {
    if (!c->frame.und_init) return fail(-1, "ldso_ct_undistort_init not called");
    if (bits != 8 && bits != 16) return fail(-1, "bits must be 8 or 16");
    const bool valid = c->frame.und_g_depth > 0;
    if (!valid || exposure_time <= 0 || c->frame.und_mode == 0)
        mode = kUndFactor;
    else
        mode = c->frame.und_mode == 2 ? kUndLutVignette : kUndLut;
    if (mode != kUndFactor && bits == 16 && c->frame.und_g_depth != 65536)
        return fail(-1, "a 16-bit frame indexes 65536 entries of G: g_depth is " + std::to_string(c->frame.und_g_depth));
    exposure = c->frame.und_use_exposure ? exposure_time : 1.0f;
    return 0;
}

// k_ct_undistort from the raw frame at dev_raw into d_color, on the context's stream
int launch_undistort(ldso_ct_ctx *c, const void *dev_raw, int bits, int mode, float factor) {
    const int n = c->pyr.w * c->pyr.h, nb = (n + kCtThreads - 1) / kCtThreads;
    const UndParams U{c->frame.d_und_remap.p, c->frame.d_und_g.p, c->frame.d_und_vinv.p, c->frame.und_w_org, n, mode, factor};
    float *out = c->frame.d_color.p;
    if (bits == 8) {
        const uint8_t *raw = static_cast<const uint8_t *>(dev_raw);
        if (c->frame.und_pass)
            k_ct_undistort<uint8_t, true><<<nb, kCtThreads, 0, c->stream>>>(raw, out, U);
        else
            k_ct_undistort<uint8_t, false><<<nb, kCtThreads, 0, c->stream>>>(raw, out, U);
    } else {
        const uint16_t *raw = static_cast<const uint16_t *>(dev_raw);
        if (c->frame.und_pass)
            k_ct_undistort<uint16_t, true><<<nb, kCtThreads, 0, c->stream>>>(raw, out, U);
        else
            k_ct_undistort<uint16_t, false><<<nb, kCtThreads, 0, c->stream>>>(raw, out, U);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-2, std::string("launch k_ct_undistort: ") + hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

int ldso_ct_set_new_frame(ldso_ct_ctx *c, const float *color, double ab_exposure, const float *b_response) {
    if (!c || !color) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    const PyrParams &P = c->pyr;
    HIP_TRY(hipMemcpyAsync(c->frame.d_color.p, color, (size_t)P.w * P.h * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const int rc = frame_pyramid(c, b_response);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's buffers may be reused on return
    c->frame.exposure = (float)ab_exposure;
    c->frame.have = true;
    return 0;
}

int ldso_ct_undistort_init(ldso_ct_ctx *c, const ldso_ct_undistort_desc *d, int32_t *n_outside_out) {
    if (!c || !d) return fail(-1, "null argument");
    if (d->w_org < 2 || d->h_org < 2) return fail(-1, "the raw image must be at least 2 x 2");
    if ((d->remap_x == nullptr) != (d->remap_y == nullptr)) return fail(-1, "remap_x and remap_y come together: one of them is NULL");
    if (d->photometric_mode < 0 || d->photometric_mode > 2) return fail(-1, "photometric_mode out of range [0, 2]");
    if (d->g && d->g_depth < 256) return fail(-1, "g_depth must be at least 256");
    if (d->g && !d->vignette_inv) return fail(-1, "g needs vignette_inv: the photometric calibration is valid with both only");
    const PyrParams &P = c->pyr;
    const bool pass = !d->remap_x;
    if (pass && (d->w_org != P.w || d->h_org != P.h))
        return fail(-1, "passthrough needs a raw image of the context's size " + std::to_string(P.w) + "x" + std::to_string(P.h));
    if ((int64_t)d->w_org * d->h_org > INT32_MAX / 2) return fail(-1, "the raw image is too large");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // no launch still reads the tables this call replaces
    c->frame.und_init = false;
    const size_t n = (size_t)P.w * P.h, n_org = (size_t)d->w_org * d->h_org;
    int rc, outside = 0;
    if (!pass) {
        // the footprint rule (include/ldso_ct.h): what the kernel would read outside the source becomes -1
        std::vector<float2> m(n);
        for (size_t i = 0; i < n; i++) {
            const float xx = d->remap_x[i], yy = d->remap_y[i];
            m[i] = make_float2(xx, yy);
            if (xx < 0) continue;  // the reference's own mark: its pixel is 0
            bool inside = std::isfinite(xx) && std::isfinite(yy) && xx < (float)d->w_org && yy > -1.0f && yy < (float)d->h_org;
            if (inside) {
                const int xxi = (int)xx, yyi = (int)yy;
                inside = xxi + 1 <= d->w_org - 1 && yyi >= 0 && yyi + 1 <= d->h_org - 1;
            }
            if (!inside) {
                m[i] = make_float2(-1.0f, -1.0f);
                outside++;
            }
        }
        if ((rc = c->frame.d_und_remap.ensure(n))) return rc;
        HIP_TRY(hipMemcpy(c->frame.d_und_remap.p, m.data(), n * sizeof(float2), hipMemcpyHostToDevice));
    }
    if (d->g) {
        if ((rc = c->frame.d_und_g.ensure((size_t)d->g_depth)) || (rc = c->frame.d_und_vinv.ensure(n_org))) return rc;
        HIP_TRY(hipMemcpy(c->frame.d_und_g.p, d->g, (size_t)d->g_depth * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->frame.d_und_vinv.p, d->vignette_inv, n_org * sizeof(float), hipMemcpyHostToDevice));
    }
    if ((rc = c->frame.h_und_raw.ensure(n_org * 2)) || (rc = c->frame.d_und_raw.ensure(n_org * 2))) return rc;
    c->frame.und_pass = pass;
    c->frame.und_w_org = d->w_org;
    c->frame.und_h_org = d->h_org;
    c->frame.und_g_depth = d->g ? d->g_depth : 0;
    c->frame.und_mode = d->photometric_mode;
    c->frame.und_use_exposure = d->use_exposure != 0;
    c->frame.und_init = true;
    if (n_outside_out) *n_outside_out = outside;
    return 0;
}

int ldso_ct_set_new_frame_raw(ldso_ct_ctx *c, const void *raw, int32_t bits, float exposure_time, float factor,
                              const float *b_response, float *exposure_out) {
    if (!c || !raw) return fail(-1, "null argument");
    int mode;
    float exposure;
    int rc = und_frame_mode(c, bits, exposure_time, mode, exposure);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // every use of the pinned frame ends behind a synchronisation, so it is free here
    const size_t bytes = (size_t)c->frame.und_w_org * c->frame.und_h_org * (bits / 8);
    std::memcpy(c->frame.h_und_raw.p, raw, bytes);
    HIP_TRY(hipMemcpyAsync(c->frame.d_und_raw.p, c->frame.h_und_raw.p, bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_undistort(c, c->frame.d_und_raw.p, bits, mode, factor)) || (rc = frame_pyramid(c, b_response))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->frame.exposure = exposure;
    c->frame.have = true;
    if (exposure_out) *exposure_out = exposure;
    return 0;
}

int ldso_ct_set_new_frame_raw_device(ldso_ct_ctx *c, const void *dev_raw, int32_t bits, float exposure_time, float factor,
                                     const float *b_response, void *producer_stream, float *exposure_out) {
    if (!c || !dev_raw) return fail(-1, "null argument");
    int mode;
    float exposure;
    int rc = und_frame_mode(c, bits, exposure_time, mode, exposure);
    if (rc) return rc;
    if (bits == 16 && (reinterpret_cast<uintptr_t>(dev_raw) & 1)) return fail(-1, "a 16-bit device source must be 2-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t prod = static_cast<hipStream_t>(producer_stream);
    // read the raw frame behind what the producer's stream holds now; the producer may overwrite its
    // buffer once the one reader of it has run
    if ((rc = c->frame.borrow.begin(c->stream, prod)) || (rc = launch_undistort(c, dev_raw, bits, mode, factor)) ||
        (rc = c->frame.borrow.end(c->stream, prod)))
        return rc;
    if ((rc = frame_pyramid(c, b_response))) return rc;
    c->frame.exposure = exposure;
    c->frame.have = true;
    if (exposure_out) *exposure_out = exposure;
    return 0;
}

int ldso_ct_get_undistorted(ldso_ct_ctx *c, float *image) {
    if (!c || !image) return fail(-1, "null argument");
    if (!c->frame.have) return fail(-1, "ldso_ct_set_new_frame not called");
    HIP_TRY(hipSetDevice(c->device));
    return ct_read(c, image, c->frame.d_color.p, (size_t)c->pyr.w * c->pyr.h);
}

int ldso_ct_get_frame_level(ldso_ct_ctx *c, int32_t lvl, float *dI, float *abs_sq_grad) {
    if (!c) return fail(-1, "null context");
    if (lvl < 0 || lvl >= c->levels) return fail(-1, "pyramid level out of range");
    if (!c->frame.have) return fail(-1, "ldso_ct_set_new_frame not called");
    const int n = c->pyr.wl[lvl] * c->pyr.hl[lvl];
    std::vector<float4> tmp(n);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ct_read(c, tmp.data(), c->frame.d_dIp.p + c->pyr.off[lvl], n)) return rc;
    for (int i = 0; i < n; i++) {
        if (dI) {
            dI[3 * i] = tmp[i].x;
            dI[3 * i + 1] = tmp[i].y;
            dI[3 * i + 2] = tmp[i].z;
        }
        if (abs_sq_grad) abs_sq_grad[i] = tmp[i].w;
    }
    return 0;
}

}  // extern "C"
