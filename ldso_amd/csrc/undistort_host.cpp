// undistort_host.cpp -- the arithmetic of the reference's Undistort constructors on the host, without a
// context: the remap tables and the rectified K (readFromFile's numeric part, makeOptimalK_crop and the
// five models' distortCoordinates; Undistort.cc:558-668, 738-751, 802-868, 891-1125) and the photometric
// tables (Undistort.cc:86-103, 120-154).  They run once per camera.  Every statement keeps the reference's
// types: a double literal lifts its expression to double, a float variable rounds it back (-ffp-contract=off).
// tanf / atanf / atan2f / sqrtf are the host libm's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ldso_ct.h"
#include "ldso_ba_internal.h"

namespace {

int fail(int code, const std::string &msg) { return ldso_ba::set_error(code, msg); }

// the reference's Undistort while it builds its tables: parsOrg, the sizes and K (Mat33, double)
struct Und {
    int model;
    double pars[8];
    int wOrg, hOrg, w, h;
    double K00 = 1, K11 = 1, K02 = 0, K12 = 0;

    void distort(float *xs, float *ys, int n) const {
        const float fx = pars[0], fy = pars[1], cx = pars[2], cy = pars[3];
        const float ofx = K00, ofy = K11, ocx = K02, ocy = K12;
        if (model == LDSO_CT_UNDISTORT_FOV) {  // :891-922
            const float dist = pars[4];
            const float d2t = 2.0f * tanf(dist / 2.0f);
            for (int i = 0; i < n; i++) {
                float ix = (xs[i] - ocx) / ofx;
                float iy = (ys[i] - ocy) / ofy;
                const float r = sqrtf(ix * ix + iy * iy);
                const float fac = (r == 0 || dist == 0) ? 1 : atanf(r * d2t) / (dist * r);
                xs[i] = fx * fac * ix + cx;
                ys[i] = fy * fac * iy + cy;
            }
        } else if (model == LDSO_CT_UNDISTORT_RADTAN) {  // :937-977
            const float k1 = pars[4], k2 = pars[5], r1 = pars[6], r2 = pars[7];
            for (int i = 0; i < n; i++) {
                const float ix = (xs[i] - ocx) / ofx;
                const float iy = (ys[i] - ocy) / ofy;
                const float mx2 = ix * ix, my2 = iy * iy, mxy = ix * iy;
                const float rho2 = mx2 + my2;
                const float rad = k1 * rho2 + k2 * rho2 * rho2;
                // the tangential terms in double: 2.0 lifts them
                const float xd = ix + ix * rad + 2.0 * r1 * mxy + r2 * (rho2 + 2.0 * mx2);
                const float yd = iy + iy * rad + 2.0 * r2 * mxy + r1 * (rho2 + 2.0 * my2);
                xs[i] = fx * xd + cx;
                ys[i] = fy * yd + cy;
            }
        } else if (model == LDSO_CT_UNDISTORT_EQUIDISTANT) {  // :992-1031
            const float k1 = pars[4], k2 = pars[5], k3 = pars[6], k4 = pars[7];
            for (int i = 0; i < n; i++) {
                const float ix = (xs[i] - ocx) / ofx;
                const float iy = (ys[i] - ocy) / ofy;
                const float r = sqrtf(ix * ix + iy * iy);
                const float theta = atanf(r);
                const float theta2 = theta * theta, theta4 = theta2 * theta2;
                const float theta6 = theta4 * theta2, theta8 = theta4 * theta4;
                const float thetad = theta * (1 + k1 * theta2 + k2 * theta4 + k3 * theta6 + k4 * theta8);
                const float scaling = (r > 1e-8) ? thetad / r : 1.0;
                xs[i] = fx * ix * scaling + cx;
                ys[i] = fy * iy * scaling + cy;
            }
        } else if (model == LDSO_CT_UNDISTORT_KANNALA_BRANDT) {  // :1046-1089
            const float k0 = pars[4], k1 = pars[5], k2 = pars[6], k3 = pars[7];
            for (int i = 0; i < n; i++) {
                const float ix = (xs[i] - ocx) / ofx;
                const float iy = (ys[i] - ocy) / ofy;
                const float rr = sqrtf(ix * ix + iy * iy);
                const float theta = atan2f(rr, 1);
                const float theta2 = theta * theta, theta3 = theta2 * theta, theta5 = theta3 * theta2;
                const float theta7 = theta5 * theta2, theta9 = theta7 * theta2;
                const float r = theta + k0 * theta3 + k1 * theta5 + k2 * theta7 + k3 * theta9;
                if (rr < 1e-6) {
                    xs[i] = fx * ix + cx;
                    ys[i] = fy * iy + cy;
                } else {
                    xs[i] = (r / rr) * fx * ix + cx;
                    ys[i] = (r / rr) * fy * iy + cy;
                }
            }
        } else {  // Pinhole, :1103-1125
            for (int i = 0; i < n; i++) {
                float ix = (xs[i] - ocx) / ofx;
                float iy = (ys[i] - ocy) / ofy;
                xs[i] = fx * ix + cx;
                ys[i] = fy * iy + cy;
            }
        }
    }

    // makeOptimalK_crop (:558-668); false where the reference gives up and exits
    bool optimal_k_crop() {
        K00 = K11 = 1;
        K02 = K12 = 0;
        const int N = 100000;
        std::vector<float> tgX(N), tgY(N);
        float minX = 0, maxX = 0, minY = 0, maxY = 0;
        // 1. the centre lines, stretched as far as they stay inside the source
        for (int x = 0; x < N; x++) {
            tgX[x] = (x - 50000.0f) / 10000.0f;
            tgY[x] = 0;
        }
        distort(tgX.data(), tgY.data(), N);
        for (int x = 0; x < N; x++)
            if (tgX[x] > 0 && tgX[x] < wOrg - 1) {
                if (minX == 0) minX = (x - 50000.0f) / 10000.0f;
                maxX = (x - 50000.0f) / 10000.0f;
            }
        for (int y = 0; y < N; y++) {
            tgY[y] = (y - 50000.0f) / 10000.0f;
            tgX[y] = 0;
        }
        distort(tgX.data(), tgY.data(), N);
        for (int y = 0; y < N; y++)
            if (tgY[y] > 0 && tgY[y] < hOrg - 1) {
                if (minY == 0) minY = (y - 50000.0f) / 10000.0f;
                maxY = (y - 50000.0f) / 10000.0f;
            }
        minX *= 1.01;
        maxX *= 1.01;
        minY *= 1.01;
        maxY *= 1.01;
        // 2. shrink the side whose border has pixels outside; of two candidates the wider dimension
        std::vector<float> rx(2 * (size_t)std::max(w, h)), ry(rx.size());
        bool oobLeft = true, oobRight = true, oobTop = true, oobBottom = true;
        int iteration = 0;
        while (oobLeft || oobRight || oobTop || oobBottom) {
            oobLeft = oobRight = oobTop = oobBottom = false;
            for (int y = 0; y < h; y++) {
                rx[y * 2] = minX;
                rx[y * 2 + 1] = maxX;
                ry[y * 2] = ry[y * 2 + 1] = minY + (maxY - minY) * (float)y / ((float)h - 1.0f);
            }
            distort(rx.data(), ry.data(), 2 * h);
            for (int y = 0; y < h; y++) {
                if (!(rx[2 * y] > 0 && rx[2 * y] < wOrg - 1)) oobLeft = true;
                if (!(rx[2 * y + 1] > 0 && rx[2 * y + 1] < wOrg - 1)) oobRight = true;
            }
            for (int x = 0; x < w; x++) {
                ry[x * 2] = minY;
                ry[x * 2 + 1] = maxY;
                rx[x * 2] = rx[x * 2 + 1] = minX + (maxX - minX) * (float)x / ((float)w - 1.0f);
            }
            distort(rx.data(), ry.data(), 2 * w);
            for (int x = 0; x < w; x++) {
                if (!(ry[2 * x] > 0 && ry[2 * x] < hOrg - 1)) oobTop = true;
                if (!(ry[2 * x + 1] > 0 && ry[2 * x + 1] < hOrg - 1)) oobBottom = true;
            }
            if ((oobLeft || oobRight) && (oobTop || oobBottom)) {
                if ((maxX - minX) > (maxY - minY))
                    oobBottom = oobTop = false;
                else
                    oobLeft = oobRight = false;
            }
            if (oobLeft) minX *= 0.995;
            if (oobRight) maxX *= 0.995;
            if (oobTop) minY *= 0.995;
            if (oobBottom) maxY *= 0.995;
            iteration++;
            if (iteration > 500) return false;
        }
        K00 = ((float)w - 1.0f) / (maxX - minX);
        K11 = ((float)h - 1.0f) / (maxY - minY);
        K02 = -minX * K00;
        K12 = -minY * K11;
        return true;
    }
};

}  // namespace

extern "C" {

int ldso_ct_undistort_make_remap(int32_t model, const double pars[8], int32_t w_org, int32_t h_org, int32_t w, int32_t h,
                                 int32_t out_mode, const float out_calib[4], double K_out[4], float *remap_x,
                                 float *remap_y, int32_t *passthrough_out) {
    if (!pars || !K_out || !remap_x || !remap_y || !passthrough_out) return fail(-1, "null argument");
    if (model < LDSO_CT_UNDISTORT_FOV || model > LDSO_CT_UNDISTORT_PINHOLE) return fail(-1, "unknown camera model");
    if (out_mode == LDSO_CT_UNDISTORT_OUT_FULL) return fail(-1, "rectification mode full is not built: the reference asserts false there");
    if (out_mode < LDSO_CT_UNDISTORT_OUT_CROP || out_mode > LDSO_CT_UNDISTORT_OUT_FULL) return fail(-1, "unknown rectification mode");
    if (w_org < 2 || h_org < 2 || w < 2 || h < 2) return fail(-1, "sizes must be at least 2 x 2");
    if ((int64_t)w * h > INT32_MAX / 2) return fail(-1, "the output image is too large");
    if (out_mode == LDSO_CT_UNDISTORT_OUT_CALIB && !out_calib) return fail(-1, "rectification to a given K needs out_calib");
    if (out_mode == LDSO_CT_UNDISTORT_OUT_NONE && (w != w_org || h != h_org))
        return fail(-1, "rectification mode none requires input and output dimensions to match");
    Und u;
    u.model = model;
    const int n_pars = (model == LDSO_CT_UNDISTORT_FOV || model == LDSO_CT_UNDISTORT_PINHOLE) ? 5 : 8;
    for (int i = 0; i < 8; i++) u.pars[i] = i < n_pars ? pars[i] : 0.0;
    u.wOrg = w_org;
    u.hOrg = h_org;
    u.w = w;
    u.h = h;
    if (u.pars[2] < 1 && u.pars[3] < 1) {  // the relative format (:738-751)
        u.pars[0] = u.pars[0] * w_org;
        u.pars[1] = u.pars[1] * h_org;
        u.pars[2] = u.pars[2] * w_org - 0.5;
        u.pars[3] = u.pars[3] * h_org - 0.5;
    }
    int pass = 0;
    if (out_mode == LDSO_CT_UNDISTORT_OUT_CROP) {
        if (!u.optimal_k_crop()) return fail(-1, "makeOptimalK_crop found no camera matrix within 500 rounds");
    } else if (out_mode == LDSO_CT_UNDISTORT_OUT_NONE) {
        u.K00 = u.pars[0];
        u.K11 = u.pars[1];
        u.K02 = u.pars[2];
        u.K12 = u.pars[3];
        pass = 1;
    } else {  // :826-830: the float products, the half pixel in double
        u.K00 = out_calib[0] * w;
        u.K11 = out_calib[1] * h;
        u.K02 = out_calib[2] * w - 0.5;
        u.K12 = out_calib[3] * h - 0.5;
    }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            remap_x[x + y * w] = x;
            remap_y[x + y * w] = y;
        }
    u.distort(remap_x, remap_y, h * w);
    const int wOrg = w_org, hOrg = h_org;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            // "make rounding resistant" (:851-867), verbatim: the fourth line sets ix, the last bound is wOrg's
            float ix = remap_x[x + y * w];
            float iy = remap_y[x + y * w];
            if (ix == 0) ix = 0.001;
            if (iy == 0) iy = 0.001;
            if (ix == wOrg - 1) ix = wOrg - 1.001;
            if (iy == hOrg - 1) ix = hOrg - 1.001;
            if (ix > 0 && iy > 0 && ix < wOrg - 1 && iy < wOrg - 1) {
                remap_x[x + y * w] = ix;
                remap_y[x + y * w] = iy;
            } else {
                remap_x[x + y * w] = -1;
                remap_y[x + y * w] = -1;
            }
        }
    K_out[0] = u.K00;
    K_out[1] = u.K11;
    K_out[2] = u.K02;
    K_out[3] = u.K12;
    *passthrough_out = pass;
    return 0;
}

int ldso_ct_undistort_make_photometric(const float *g_raw, int32_t g_depth, const void *vignette, int32_t vignette_bits,
                                       int32_t n, int32_t photometric_mode, float *g_out, float *vignette_inv_out) {
    if (!g_raw || !vignette || !g_out || !vignette_inv_out) return fail(-1, "null argument");
    if (g_depth < 256) return fail(-1, "g_depth must be at least 256");
    if (vignette_bits != 8 && vignette_bits != 16) return fail(-1, "vignette_bits must be 8 or 16");
    if (n < 1) return fail(-1, "the vignette image is empty");
    if (photometric_mode < 0 || photometric_mode > 2) return fail(-1, "photometric_mode out of range [0, 2]");
    for (int i = 0; i < g_depth - 1; i++)
        if (g_raw[i + 1] <= g_raw[i]) return fail(-1, "G has to be strictly increasing");
    const float min = g_raw[0], max = g_raw[g_depth - 1];
    for (int i = 0; i < g_depth; i++) g_out[i] = 255.0 * (g_raw[i] - min) / (max - min);  // :98
    if (photometric_mode == 0)
        for (int i = 0; i < g_depth; i++) g_out[i] = 255.0f * i / (float)(g_depth - 1);  // :102
    const uint8_t *v8 = static_cast<const uint8_t *>(vignette);
    const uint16_t *v16 = static_cast<const uint16_t *>(vignette);
    float maxV = 0;
    for (int i = 0; i < n; i++) {
        const int v = vignette_bits == 16 ? v16[i] : v8[i];
        if (v > maxV) maxV = v;
    }
    for (int i = 0; i < n; i++) {
        const int v = vignette_bits == 16 ? v16[i] : v8[i];
        const float map = v / maxV;
        vignette_inv_out[i] = 1.0f / map;
    }
    return 0;
}

}  // extern "C"
