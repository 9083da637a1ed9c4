// ct_host_ip.h -- immature points: make, upload, download, append and trace (k_ct_immature.h).  Owns c->ip.  Reads
// frame.d_dIp / d_inten; ldso_ct_make_immature fills the core's d_mk.
// A piece of the one translation unit ldso_ct.hip (k_ct_pyramid.h).
#pragma once
#include <algorithm>
#include <cstring>

#include "ct_context.h"

#pragma clang fp contract(off)

extern "C" {

int ldso_ct_make_immature(ldso_ct_ctx *c, int32_t n, const float *uv, float type, int32_t host,
                          ldso_ct_immature *out) {
    if (!c) return fail(-1, "null context");
    if (n < 0 || (n > 0 && (!uv || !out))) return fail(-1, "bad point arguments");
    if (!c->frame.have) return fail(-1, "ldso_ct_set_new_frame has not been called");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    // (the stream is idle: every call that uses these buffers ends with a synchronisation)
    int rc;
    if ((rc = c->ip.d_uv.ensure(n)) || (rc = c->d_mk.ensure(n))) return rc;
    HIP_TRY(hipMemcpyAsync(c->ip.d_uv.p, uv, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    const int w = c->pyr.w, h = c->pyr.h;
    rc = ct_launch(c, kCtSlotMakeImmature, [&] {
        k_ct_make_immature<<<(n + kCtThreads - 1) / kCtThreads, kCtThreads, 0, c->stream>>>(
            c->frame.d_dIp.p, w, h, n, c->ip.d_uv.p, type, host, c->d_mk.p);
    });
    if (rc) return rc;
    return ct_read(c, out, c->d_mk.p, n);
}

int ldso_ct_immature_upload(ldso_ct_ctx *c, int32_t n, const ldso_ct_immature *pts) {
    if (!c) return fail(-1, "null context");
    if (n < 0 || (n > 0 && !pts)) return fail(-1, "bad point arguments");
    int max_host = -1;
    for (int k = 0; k < n; k++) {
        if (pts[k].host < 0) return fail(-1, "immature point with a negative host index");
        if (pts[k].last_status < 0 || pts[k].last_status > LDSO_CT_IPS_UNINITIALIZED)
            return fail(-1, "immature point with an invalid status");
        max_host = std::max(max_host, (int)pts[k].host);
    }
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = c->ip.d_ip.ensure(n)) return rc;  // (the stream is idle, as in ldso_ct_make_immature)
    if (n) HIP_TRY(hipMemcpyAsync(c->ip.d_ip.p, pts, (size_t)n * sizeof(IpRec), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ip.n = n;
    c->ip.max_host = max_host;
    return 0;
}

int ldso_ct_immature_download(ldso_ct_ctx *c, int32_t n, ldso_ct_immature *pts) {
    if (!c) return fail(-1, "null context");
    if (n != c->ip.n) return fail(-1, "count differs from the resident immature points");
    if (n == 0) return 0;
    if (!pts) return fail(-1, "null output");
    HIP_TRY(hipSetDevice(c->device));
    return ct_read(c, pts, c->ip.d_ip.p, n);
}

int ldso_ct_trace(ldso_ct_ctx *c, int32_t n_hosts, const float *krki, const float *kt, const float *aff,
                  int32_t *counts_out) {
    if (!c) return fail(-1, "null context");
    if (!c->frame.have) return fail(-1, "ldso_ct_set_new_frame has not been called");
    if (n_hosts <= c->ip.max_host) return fail(-1, "an immature point's host index is >= n_hosts");
    if (n_hosts > 0 && (!krki || !kt || !aff)) return fail(-1, "null host tables");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n_tab = (size_t)n_hosts * kHostStride;
    int rc;
    if (n_hosts > 0 && ((rc = c->ip.d_hosts.ensure(n_tab)) || (rc = c->ip.h_hosts.ensure(n_tab)))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the staging buffer may still feed a previous copy
    for (int i = 0; i < n_hosts; i++) {
        float *o = c->ip.h_hosts.p + (size_t)i * kHostStride;
        std::memcpy(o, krki + 9 * (size_t)i, 9 * sizeof(float));
        std::memcpy(o + 9, kt + 3 * (size_t)i, 3 * sizeof(float));
        o[12] = aff[2 * (size_t)i];
        o[13] = aff[2 * (size_t)i + 1];
        o[14] = o[15] = 0;
    }
    if (n_hosts)
        HIP_TRY(hipMemcpyAsync(c->ip.d_hosts.p, c->ip.h_hosts.p, (size_t)n_hosts * kHostStride * sizeof(float),
                              hipMemcpyHostToDevice, c->stream));
    const int n = c->ip.n;
    if (n > 0) {
        TraceParams P{c->frame.d_dIp.p, c->frame.d_inten.p, c->ip.d_hosts.p, c->ip.d_ip.p, n, c->pyr.w, c->pyr.h};
        const int per = kCtThreads / kWave;
        rc = ct_launch(c, kCtSlotTrace, [&] { k_ct_trace<<<(n + per - 1) / per, kCtThreads, 0, c->stream>>>(P); });
        if (rc) return rc;
    }
    if (counts_out) {
        rc = ct_launch(c, kCtSlotIpCount, [&] { k_ct_ip_count<<<1, 1024, 0, c->stream>>>(c->ip.d_ip.p, n, c->ip.d_counts.p); });
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(c->ip.h_counts.p, c->ip.d_counts.p, 6 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (counts_out) std::memcpy(counts_out, c->ip.h_counts.p, 6 * sizeof(int));
    return 0;
}

int ldso_ct_immature_append(ldso_ct_ctx *c, int32_t n, const ldso_ct_immature *pts) {
    if (!c) return fail(-1, "null context");
    if (n < 0 || (n > 0 && !pts)) return fail(-1, "bad point arguments");
    int max_host = c->ip.max_host;
    for (int k = 0; k < n; k++) {
        if (pts[k].host < 0) return fail(-1, "immature point with a negative host index");
        if (pts[k].last_status < 0 || pts[k].last_status > LDSO_CT_IPS_UNINITIALIZED)
            return fail(-1, "immature point with an invalid status");
        max_host = std::max(max_host, (int)pts[k].host);
    }
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    const size_t need = (size_t)c->ip.n + n;
    if (c->ip.d_ip.n < need || !c->ip.d_ip.p) {
        // a larger buffer with room to spare, the resident records moved over on the device
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (int rc = c->ip.d_ip_alt.alloc(std::max(need, 2 * c->ip.d_ip.n))) return rc;
        if (c->ip.n)
            HIP_TRY(hipMemcpyAsync(c->ip.d_ip_alt.p, c->ip.d_ip.p, (size_t)c->ip.n * sizeof(IpRec), hipMemcpyDeviceToDevice,
                                   c->stream));
        std::swap(c->ip.d_ip.p, c->ip.d_ip_alt.p);
        std::swap(c->ip.d_ip.n, c->ip.d_ip_alt.n);
    }
    HIP_TRY(hipMemcpyAsync(c->ip.d_ip.p + c->ip.n, pts, (size_t)n * sizeof(IpRec), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ip.n += n;
    c->ip.max_host = max_host;
    return 0;
}

}  // extern "C"
