// ims_opd.h -- optical path difference (wavefront) maps and their annular-Zernike normal equations (ims_opd, the `opd` extra
// output of imsim/opd.py, which calls batoid's wavefront and zernike).
//
// All arithmetic is binary64, one thread per ray or pixel, 256-thread workgroups.  The launches of one call:
//   k_opd_trace        every ray of every field (pixels first, then one chief ray per field from the stop centre) through the
//                      optics with trace_step<-1, -1, true> (Newton to f64 resolution); optical path n_in (d . r) at the start,
//                      plus n_before |step| per surface; detector hit, unit direction, path, index at the detector and status
//   k_opd_hit_partial  (mean reference only) per-workgroup sums of the unvignetted detector hits
//   k_opd_field        one workgroup per field: the reference point (chief hit, or the mean hit)
//   k_opd_sphere       each ray back to the reference sphere, t = path + n_det s (s < 0), kept as t - t_chief, with the
//                      per-workgroup sums of the unvignetted rays' values
//   k_opd_field        one workgroup per field: t0 - t_chief (0 for the chief reference, the mean of the unvignetted rays else)
//   k_opd_map          OPD = (t0 - t) 1e9 nm, NaN where the ray was vignetted or lost
//   k_opd_zk_normal    per (field, chunk of 4096 pixels): partial A^T A and A^T w over the finite pixels, A_pj = Z_j(pixel p)
//   k_opd_zk_final     per (field, entry): the chunks' partials summed in chunk order
// Every sum has a fixed shape (a workgroup's tree over its 256 threads, then the partials in index order), so the results depend
// neither on the launch geometry nor on which other fields share the call.
//
// A section of the one translation unit (imsim_hip.hip): the kernels in namespace ims, then the host side -- opd_run,
// trace_field_points_run; entry points ims_opd, ims_opd_perturbed, ims_trace_field_points, ims_trace_field_points_perturbed.
#pragma once
#include "ims_photon.h"

namespace ims {

constexpr int OPD_WG = 256;
constexpr int OPD_CHUNK = 4096;     // pixels per workgroup of k_opd_zk_normal (IMS_OPD_CHUNKS)
constexpr int OPD_TILE = 64;        // pixels whose Zernike values sit in LDS at a time
constexpr int OPD_REC = 10;         // doubles per ray record: pos[3], dir[3], path, n_det, t - t_chief, status
constexpr int OPD_MAX_ENT = IMS_OPD_MAX_J * (IMS_OPD_MAX_J + 3) / 2;
constexpr int OPD_ENT_PER_THREAD = (OPD_MAX_ENT + OPD_WG - 1) / OPD_WG;

// scratch layout (IMS_OPD_SCRATCH_BYTES): ray records (structure of arrays), hit partials [field][block][4], t partials
// [field][block][2], per-field values [field][4] (reference point, t0 - t_chief), Zernike partials [field][chunk][entry]
struct OpdLayout {
    int64_t npix, n_rays, nblk, nchunk, nent;
    double* rec;
    double* hit_part;
    double* t_part;
    double* field;
    double* zk_part;
};

inline OpdLayout opd_layout(const ims_opd_t& P)
{
    OpdLayout L;
    L.npix = (int64_t)P.nx * P.nx;
    L.n_rays = (int64_t)P.n_fields * (L.npix + 1);
    L.nblk = IMS_OPD_BLOCKS(P.nx);
    L.nchunk = IMS_OPD_CHUNKS(P.nx);
    L.nent = (int64_t)P.jmax * (P.jmax + 3) / 2;
    double* s = (double*)P.scratch;
    L.rec = s;
    L.hit_part = L.rec + OPD_REC * L.n_rays;
    L.t_part = L.hit_part + (int64_t)P.n_fields * L.nblk * 4;
    L.field = L.t_part + (int64_t)P.n_fields * L.nblk * 2;
    L.zk_part = L.field + (int64_t)P.n_fields * 4;
    return L;
}

// the sum of v over the workgroup, in a fixed tree order; every thread gets it
IMS_DEV double opd_block_sum(double v, double* lds)
{
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int h = OPD_WG / 2; h > 0; h >>= 1) {
        if (tid < h) lds[tid] = lds[tid] + lds[tid + h];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

// ray r: pixel p = r mod npix of field r / npix for r < n_fields npix, else the chief ray of field r - n_fields npix
// PERT: `optics` is an ims_optics_perturbed_t and every surface goes through trace_step_pert (in telescope coordinates
// throughout: the path lengths and the reference sphere do not depend on the frame they are measured in)
template <bool PERT = false>
__global__ __launch_bounds__(256) void k_opd_trace(const ims_opd_t P, const ims_optics_t* __restrict__ optics, OpdLayout L)
{
    const int64_t r = (int64_t)blockIdx.x * OPD_WG + threadIdx.x;
    if (r >= L.n_rays) return;
    const ims_optics_t& o = *optics;
    const int64_t n_pix_rays = (int64_t)P.n_fields * L.npix;
    int64_t f;
    double x = 0.0, y = 0.0;
    if (r < n_pix_rays) {
        f = r / L.npix;
        const int64_t p = r - f * L.npix;
        const int64_t j = p / P.nx, i = p - j * P.nx;
        const double half = 0.5 * (double)(P.nx - 1);
        x = ((double)i - half) * P.dx;
        y = ((double)j - half) * P.dx;
    } else {
        f = r - n_pix_rays;
    }
    const double wave = P.wavelength;
    TraceState st;
    st.vignetted = 0;
    if (o.in_medium_kind == IMS_MEDIUM_CONST) st.n_cur = o.in_medium_c[0];
    else st.n_cur = medium_n(o.in_medium_kind, o.in_medium_c, wave);
    st.glass_id = -1; st.glass_n = 0.0; st.glass_in = 0.0;
    double pos[3] = { x, y, o.stop_z };
    double vel[3] = { P.dirs[3 * f], P.dirs[3 * f + 1], P.dirs[3 * f + 2] };
    // the plane wave's phase at the start, measured from the plane through the origin normal to it
    double path = st.n_cur * fma(vel[0], pos[0], fma(vel[1], pos[1], vel[2] * pos[2]));
    int status = 0;
    for (int k = 0; k < o.n_surfaces; ++k) {
        const double p0[3] = { pos[0], pos[1], pos[2] };
        const double v0[3] = { vel[0], vel[1], vel[2] };
        const double n_seg = st.n_cur;               // the medium the ray crosses to reach surface k
        if (PERT) {
            if (!trace_step_pert(o.surf[k], perturbation_of(o).surf[k], st, pos, vel, wave, false)) { status = 2; break; }
        } else if (!trace_step<-1, -1, true>(o.surf[k], st, pos, vel, wave)) { status = 2; break; }
        const double d0 = pos[0] - p0[0], d1 = pos[1] - p0[1], d2 = pos[2] - p0[2];
        double len = sqrt(fma(d0, d0, fma(d1, d1, d2 * d2)));
        if (fma(d0, v0[0], fma(d1, v0[1], d2 * v0[2])) < 0.0) len = -len;     // a surface behind the ray: negative path
        path = fma(n_seg, len, path);
    }
    if (status == 0 && st.vignetted) status = 1;
    const double vn = sqrt(fma(vel[0], vel[0], fma(vel[1], vel[1], vel[2] * vel[2])));
    double* rec = L.rec;
    const int64_t n = L.n_rays;
    rec[r] = pos[0]; rec[n + r] = pos[1]; rec[2 * n + r] = pos[2];
    rec[3 * n + r] = vel[0] / vn; rec[4 * n + r] = vel[1] / vn; rec[5 * n + r] = vel[2] / vn;
    rec[6 * n + r] = path;
    rec[7 * n + r] = st.n_cur;
    rec[9 * n + r] = (double)status;
}

// grid (nblk, n_fields): sums of x, y, z and the count of the unvignetted rays of a block of 256 pixels
__global__ __launch_bounds__(256) void k_opd_hit_partial(const ims_opd_t P, OpdLayout L)
{
    __shared__ double lds[OPD_WG];
    const int64_t f = blockIdx.y, b = blockIdx.x;
    const int64_t p = b * OPD_WG + threadIdx.x;
    const int64_t r = f * L.npix + p;
    const int64_t n = L.n_rays;
    const bool good = p < L.npix && L.rec[9 * n + r] == 0.0;
    double* out = L.hit_part + (f * L.nblk + b) * 4;
    for (int c = 0; c < 3; ++c) {
        const double s = opd_block_sum(good ? L.rec[c * n + r] : 0.0, lds);
        if (threadIdx.x == 0) out[c] = s;
    }
    const double cnt = opd_block_sum(good ? 1.0 : 0.0, lds);
    if (threadIdx.x == 0) out[3] = cnt;
}

// one workgroup per field.  stage 0: the reference point (field[0..2]); stage 1: t0 - t_chief (field[3])
__global__ __launch_bounds__(256) void k_opd_field(const ims_opd_t P, OpdLayout L, int stage)
{
    __shared__ double lds[OPD_WG];
    const int64_t f = blockIdx.x;
    double* fv = L.field + f * 4;
    const int64_t chief = (int64_t)P.n_fields * L.npix + f;
    const int64_t n = L.n_rays;
    if (P.reference == IMS_OPD_REF_CHIEF) {
        if (threadIdx.x == 0) {
            if (stage == 0) { fv[0] = L.rec[chief]; fv[1] = L.rec[n + chief]; fv[2] = L.rec[2 * n + chief]; }
            else fv[3] = 0.0;
        }
        return;
    }
    const int nv = (stage == 0) ? 4 : 2;
    const double* part = (stage == 0) ? L.hit_part : L.t_part;
    double sum[4];
    for (int c = 0; c < nv; ++c) {
        double s = 0.0;
        for (int64_t b = threadIdx.x; b < L.nblk; b += OPD_WG) s += part[(f * L.nblk + b) * nv + c];
        sum[c] = opd_block_sum(s, lds);
    }
    if (threadIdx.x != 0) return;
    const double cnt = sum[nv - 1];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (stage == 0) {
        for (int c = 0; c < 3; ++c) fv[c] = (cnt > 0.0) ? sum[c] / cnt : nan;
    } else {
        fv[3] = (cnt > 0.0) ? sum[0] / cnt : nan;
    }
}

// t of ray r on the reference sphere of its field: back along the ray from its detector hit by s < 0 with
// |hit + s d - ref| = R, t = path + n_det s; NaN if the ray was lost or misses the sphere
IMS_DEV double opd_sphere_t(const ims_opd_t& P, const OpdLayout& L, int64_t r, const double* ref)
{
    const int64_t n = L.n_rays;
    if (L.rec[9 * n + r] == 2.0) return __longlong_as_double(0x7ff8000000000000ll);
    const double w0 = L.rec[r] - ref[0], w1 = L.rec[n + r] - ref[1], w2 = L.rec[2 * n + r] - ref[2];
    const double b = fma(w0, L.rec[3 * n + r], fma(w1, L.rec[4 * n + r], w2 * L.rec[5 * n + r]));
    const double R = P.sphere_radius;
    const double c = fma(w0, w0, fma(w1, w1, w2 * w2)) - R * R;
    const double disc = fma(b, b, -c);
    if (!(disc >= 0.0)) return __longlong_as_double(0x7ff8000000000000ll);
    const double sq = sqrt(disc);
    const double s = (b >= 0.0) ? -(b + sq) : c / (sq - b);     // the negative root without cancellation
    return fma(L.rec[7 * n + r], s, L.rec[6 * n + r]);
}

// grid (nblk, n_fields): t - t_chief of every pixel ray (NaN unless the ray reached the detector unvignetted), and the
// block's sum and count of the finite values
__global__ __launch_bounds__(256) void k_opd_sphere(const ims_opd_t P, OpdLayout L)
{
    __shared__ double lds[OPD_WG];
    const int64_t f = blockIdx.y, b = blockIdx.x;
    const int64_t p = b * OPD_WG + threadIdx.x;
    const int64_t r = f * L.npix + p;
    const int64_t n = L.n_rays;
    const double* ref = L.field + f * 4;
    const double t_chief = opd_sphere_t(P, L, (int64_t)P.n_fields * L.npix + f, ref);
    double v = __longlong_as_double(0x7ff8000000000000ll);
    if (p < L.npix && L.rec[9 * n + r] == 0.0) v = opd_sphere_t(P, L, r, ref) - t_chief;
    if (p < L.npix) L.rec[8 * n + r] = v;
    const bool fin = v == v;
    const double s = opd_block_sum(fin ? v : 0.0, lds);
    const double cnt = opd_block_sum(fin ? 1.0 : 0.0, lds);
    if (threadIdx.x == 0) {
        double* out = L.t_part + (f * L.nblk + b) * 2;
        out[0] = s; out[1] = cnt;
    }
}

__global__ __launch_bounds__(256) void k_opd_map(const ims_opd_t P, OpdLayout L)
{
    const int64_t q = (int64_t)blockIdx.x * OPD_WG + threadIdx.x;
    if (q >= (int64_t)P.n_fields * L.npix) return;
    const int64_t f = q / L.npix;
    P.opd[q] = (L.field[f * 4 + 3] - L.rec[8 * L.n_rays + q]) * 1.0e9;
}

// Z_j at pupil point (x, y): zk_poly row j in rho = r / r_outer times cos / sin(|m| theta) by recurrence from x / r, y / r
IMS_DEV double opd_zernike(const ims_opd_t& P, int j, double rho, double cs, double sn)
{
    const double* a = P.zk_poly + j * IMS_OPD_NPOW;
    double v = a[IMS_OPD_NPOW - 1];
    for (int k = IMS_OPD_NPOW - 2; k >= 0; --k) v = fma(v, rho, a[k]);
    const int m = P.zk_m[j];
    if (m == 0) return v;
    const int am = m > 0 ? m : -m;
    double c = cs, s = sn;
    for (int k = 1; k < am; ++k) {
        const double c2 = fma(c, cs, -(s * sn));
        s = fma(s, cs, c * sn);
        c = c2;
    }
    return v * (m > 0 ? c : s);
}

// grid (nchunk, n_fields): the chunk's partial sums of entry e of the (jmax + 1)^2 upper triangle without its last diagonal
// element, rows k < jmax: (k, l <= jmax), column jmax being the map value -- A^T A and A^T w in one packed list
__global__ __launch_bounds__(256) void k_opd_zk_normal(const ims_opd_t P, OpdLayout L)
{
    __shared__ double zt[(IMS_OPD_MAX_J + 1) * OPD_TILE];
    const int J = P.jmax;
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.y, c = blockIdx.x;
    // LDS offsets of the two rows of each of the thread's entries (entries past nent read row 0 twice; never stored)
    int kk[OPD_ENT_PER_THREAD], ll[OPD_ENT_PER_THREAD];
    double acc[OPD_ENT_PER_THREAD];
#pragma unroll
    for (int q = 0; q < OPD_ENT_PER_THREAD; ++q) {
        int e = tid + q * OPD_WG, k = 0, len = J + 1;
        while (e >= len && k < J) { e -= len; ++k; --len; }
        const bool live = tid + q * OPD_WG < L.nent;
        kk[q] = live ? k * OPD_TILE : 0; ll[q] = live ? (k + e) * OPD_TILE : 0; acc[q] = 0.0;
    }
    const int64_t p0 = c * OPD_CHUNK;
    const int64_t p1 = (p0 + OPD_CHUNK < L.npix) ? p0 + OPD_CHUNK : L.npix;
    const double half = 0.5 * (double)(P.nx - 1);
    const double inv_ro = 1.0 / P.r_outer;
    const int lane = tid & (OPD_TILE - 1);
    for (int64_t t0 = p0; t0 < p1; t0 += OPD_TILE) {
        const int64_t p = t0 + lane;
        double w = 0.0;
        bool ok = false;
        if (p < p1) {
            w = P.opd[f * L.npix + p];
            ok = w == w;
        }
        const int64_t jj = p / P.nx, ii = p - jj * P.nx;
        const double x = ((double)ii - half) * P.dx, y = ((double)jj - half) * P.dx;
        const double rr = sqrt(fma(x, x, y * y));
        const double cs = rr > 0.0 ? x / rr : 1.0, sn = rr > 0.0 ? y / rr : 0.0;
        const double rho = rr * inv_ro;
        __syncthreads();
        for (int j = tid / OPD_TILE; j < J; j += OPD_WG / OPD_TILE) zt[j * OPD_TILE + lane] = ok ? opd_zernike(P, j, rho, cs, sn) : 0.0;
        if (tid < OPD_TILE) zt[J * OPD_TILE + lane] = ok ? w : 0.0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < OPD_ENT_PER_THREAD; ++q) {
            const double* zk = zt + kk[q];
            const double* zl = zt + ll[q];
            double a = acc[q];
#pragma unroll 4
            for (int i = 0; i < OPD_TILE; ++i) a = fma(zk[i], zl[i], a);
            acc[q] = a;
        }
    }
    double* out = L.zk_part + (f * L.nchunk + c) * L.nent;
#pragma unroll
    for (int q = 0; q < OPD_ENT_PER_THREAD; ++q) {
        const int e = tid + q * OPD_WG;
        if (e < L.nent) out[e] = acc[q];
    }
}

// one thread per (field, entry): the chunks' partials in chunk order, split into A^T A (packed) and A^T w
__global__ __launch_bounds__(256) void k_opd_zk_final(const ims_opd_t P, OpdLayout L)
{
    const int64_t q = (int64_t)blockIdx.x * OPD_WG + threadIdx.x;
    if (q >= (int64_t)P.n_fields * L.nent) return;
    const int64_t f = q / L.nent;
    const int J = P.jmax;
    int e = (int)(q - f * L.nent), k = 0, len = J + 1;
    while (e >= len) { e -= len; ++k; --len; }
    const int l = k + e;
    double s = 0.0;
    for (int64_t c = 0; c < L.nchunk; ++c) s += L.zk_part[(f * L.nchunk + c) * L.nent + (q - f * L.nent)];
    if (l == J) {
        P.zk_atw[f * J + k] = s;
    } else {
        // row k of the packed upper triangle of A^T A starts at k J - k (k - 1) / 2
        P.zk_ata[f * ((int64_t)J * (J + 1) / 2) + (int64_t)k * J - (int64_t)k * (k - 1) / 2 + (l - k)] = s;
    }
}

// ---------------- batched field-point trace (ims_trace_field_points: the points a CCD's WCS is fitted through) ----------------
// One workgroup per field angle.  Thread t traces pupil rays t, t + 256, ... of the caller's table from the stop plane, every
// intersection resolved to f64 (trace_step<-1, -1, true>, or trace_step_pert with the detector hit kept in the detector's
// frame), and adds the detector hits of the rays that are neither vignetted nor lost in ray order; the workgroup's sums go
// through opd_block_sum's fixed tree in LDS, and thread 0 turns the mean hit into a pixel position the way rubin_op does
// (camera rotator, focal plane [mm] with x and y swapped, the fp_to_pix affine).  No atomics: a field's result depends
// neither on the other fields of the call nor on the run.
template <bool PERT>
__global__ __launch_bounds__(256) void k_trace_field_points(const ims_optics_t* __restrict__ optics, const double* __restrict__ thx,
                                                            const double* __restrict__ thy, double wave_nm,
                                                            const double* __restrict__ pupil_xy, int n_rays,
                                                            double* __restrict__ xy_out, int32_t* __restrict__ ngood_out)
{
    __shared__ double lds[OPD_WG];
    const ims_optics_t& o = *optics;
    const int64_t f = blockIdx.x;
    const double tx = thx[f], ty = thy[f];
    double n_in;
    if (o.in_medium_kind == IMS_MEDIUM_CONST) n_in = o.in_medium_c[0];
    else n_in = medium_n(o.in_medium_kind, o.in_medium_c, wave_nm);
    // the plane wave of field (tx, ty): direction (tx, ty, -1) / sqrt(1 + tx^2 + ty^2), speed 1 / n_in (optics.pupil_rays)
    const double g = 1.0 / sqrt(1.0 + tx * tx + ty * ty);
    const double v0[3] = { tx * g / n_in, ty * g / n_in, -g / n_in };
    double sx = 0.0, sy = 0.0, cnt = 0.0;
    for (int r = threadIdx.x; r < n_rays; r += OPD_WG) {
        TraceState st;
        st.vignetted = 0;
        st.n_cur = n_in;
        st.glass_id = -1; st.glass_n = 0.0; st.glass_in = 0.0;
        double pos[3] = { pupil_xy[2 * r], pupil_xy[2 * r + 1], o.stop_z };
        double vel[3] = { v0[0], v0[1], v0[2] };
        bool ok = true;
        for (int k = 0; k < o.n_surfaces && ok; ++k) {
            if (PERT) ok = trace_step_pert(o.surf[k], perturbation_of(o).surf[k], st, pos, vel, wave_nm, k == o.n_surfaces - 1);
            else ok = trace_step<-1, -1, true>(o.surf[k], st, pos, vel, wave_nm);
        }
        if (ok && !st.vignetted) { sx += pos[0]; sy += pos[1]; cnt += 1.0; }
    }
    sx = opd_block_sum(sx, lds);
    sy = opd_block_sum(sy, lds);
    cnt = opd_block_sum(cnt, lds);
    if (threadIdx.x != 0) return;
    ngood_out[f] = (int32_t)cnt;
    if (!(cnt > 0.0)) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        xy_out[2 * f] = nan; xy_out[2 * f + 1] = nan;
        return;
    }
    const double mx = sx / cnt, my = sy / cnt;
    const double c = o.cam_rot[0], s = o.cam_rot[1];
    const double rx = c * mx + s * my, ry = -s * mx + c * my;
    const double fpx = ry * 1.0e3, fpy = rx * 1.0e3;
    xy_out[2 * f] = o.fp_to_pix[0] * fpx + o.fp_to_pix[1] * fpy + o.fp_to_pix[2];
    xy_out[2 * f + 1] = o.fp_to_pix[3] * fpx + o.fp_to_pix[4] * fpy + o.fp_to_pix[5];
}

}  // namespace ims

extern "C" {

static int opd_run(const ims_opd_t* P, const ims_optics_t* optics_dev, bool pert, void* stream)
{
    if (!P || !optics_dev) return set_err(IMS_ERR_ARG, "opd / optics is NULL");
    if (P->n_fields < 0) return set_err(IMS_ERR_ARG, "opd: negative n_fields");
    if (P->nx < 1 || P->nx > IMS_OPD_MAX_NX) return set_err(IMS_ERR_ARG, "opd: nx out of range");
    if (P->reference != IMS_OPD_REF_CHIEF && P->reference != IMS_OPD_REF_MEAN) return set_err(IMS_ERR_ARG, "opd: unknown reference");
    if (P->jmax < 0 || P->jmax > IMS_OPD_MAX_J) return set_err(IMS_ERR_ARG, "opd: jmax out of range (0 .. 66)");
    if (!(P->dx > 0.0) || !(P->wavelength > 0.0) || !(P->sphere_radius > 0.0))
        return set_err(IMS_ERR_ARG, "opd: dx, wavelength and sphere_radius must be positive");
    if (P->n_fields == 0) return IMS_OK;
    if (!P->dirs || !P->opd || !P->scratch) return set_err(IMS_ERR_ARG, "opd: dirs / opd / scratch is NULL");
    if (P->jmax > 0) {
        if (!P->zk_poly || !P->zk_m || !P->zk_ata || !P->zk_atw) return set_err(IMS_ERR_ARG, "opd: Zernike table or output is NULL");
        if (!(P->r_outer > 0.0) || !(P->eps >= 0.0 && P->eps < 1.0)) return set_err(IMS_ERR_ARG, "opd: r_outer > 0 and 0 <= eps < 1");
    }
    const OpdLayout L = opd_layout(*P);
    if ((L.n_rays + OPD_WG - 1) / OPD_WG > 0x7fffffffLL || L.nblk > 0x7fffffffLL || P->n_fields > 65535)
        return set_err(IMS_ERR_ARG, "opd: too many rays or fields for one call");
    hipStream_t s = (hipStream_t)stream;
    const ims_opd_t A = *P;
    const dim3 per_block((unsigned)L.nblk, (unsigned)P->n_fields);
    if (pert) hipLaunchKernelGGL((k_opd_trace<true>), dim3((unsigned)((L.n_rays + OPD_WG - 1) / OPD_WG)), dim3(OPD_WG), 0, s, A, optics_dev, L);
    else hipLaunchKernelGGL((k_opd_trace<false>), dim3((unsigned)((L.n_rays + OPD_WG - 1) / OPD_WG)), dim3(OPD_WG), 0, s, A, optics_dev, L);
    if (P->reference == IMS_OPD_REF_MEAN) hipLaunchKernelGGL(k_opd_hit_partial, per_block, dim3(OPD_WG), 0, s, A, L);
    hipLaunchKernelGGL(k_opd_field, dim3((unsigned)P->n_fields), dim3(OPD_WG), 0, s, A, L, 0);
    hipLaunchKernelGGL(k_opd_sphere, per_block, dim3(OPD_WG), 0, s, A, L);
    hipLaunchKernelGGL(k_opd_field, dim3((unsigned)P->n_fields), dim3(OPD_WG), 0, s, A, L, 1);
    const int64_t n_map = (int64_t)P->n_fields * L.npix;
    hipLaunchKernelGGL(k_opd_map, dim3((unsigned)((n_map + OPD_WG - 1) / OPD_WG)), dim3(OPD_WG), 0, s, A, L);
    if (P->jmax > 0) {
        hipLaunchKernelGGL(k_opd_zk_normal, dim3((unsigned)L.nchunk, (unsigned)P->n_fields), dim3(OPD_WG), 0, s, A, L);
        const int64_t n_ent = (int64_t)P->n_fields * L.nent;
        hipLaunchKernelGGL(k_opd_zk_final, dim3((unsigned)((n_ent + OPD_WG - 1) / OPD_WG)), dim3(OPD_WG), 0, s, A, L);
    }
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_opd(const ims_opd_t* P, const ims_optics_t* optics_dev, void* stream)
{
    return opd_run(P, optics_dev, false, stream);
}

int ims_opd_perturbed(const ims_opd_t* P, const ims_optics_perturbed_t* optics_dev, void* stream)
{
    return opd_run(P, optics_dev ? &optics_dev->optics : nullptr, true, stream);
}

static int trace_field_points_run(const ims_optics_t* optics_dev, bool pert, const double* thx, const double* thy, int64_t n,
                                  double wave_nm, const double* pupil_xy, int32_t n_rays, double* xy_out, int32_t* ngood_out,
                                  void* stream)
{
    if (n < 0) return set_err(IMS_ERR_ARG, "trace_field_points: negative n");
    if (n == 0) return IMS_OK;
    if (!optics_dev || !thx || !thy || !pupil_xy || !xy_out || !ngood_out) return set_err(IMS_ERR_ARG, "trace_field_points: NULL argument");
    if (n > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "trace_field_points: too many field points for one call");
    if (n_rays < 1 || n_rays > IMS_TRACE_MAX_RAYS) return set_err(IMS_ERR_ARG, "trace_field_points: n_rays out of range");
    if (!(wave_nm > 0.0)) return set_err(IMS_ERR_ARG, "trace_field_points: the wavelength must be positive");
    hipStream_t s = (hipStream_t)stream;
    if (pert) hipLaunchKernelGGL((k_trace_field_points<true>), dim3((unsigned)n), dim3(OPD_WG), 0, s, optics_dev, thx, thy, wave_nm,
                                 pupil_xy, (int)n_rays, xy_out, ngood_out);
    else hipLaunchKernelGGL((k_trace_field_points<false>), dim3((unsigned)n), dim3(OPD_WG), 0, s, optics_dev, thx, thy, wave_nm,
                            pupil_xy, (int)n_rays, xy_out, ngood_out);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_trace_field_points(const ims_optics_t* optics_dev, const double* thx, const double* thy, int64_t n, double wave_nm,
                           const double* pupil_xy, int32_t n_rays, double* xy_out, int32_t* ngood_out, void* stream)
{
    return trace_field_points_run(optics_dev, false, thx, thy, n, wave_nm, pupil_xy, n_rays, xy_out, ngood_out, stream);
}

int ims_trace_field_points_perturbed(const ims_optics_perturbed_t* optics_dev, const double* thx, const double* thy, int64_t n,
                                     double wave_nm, const double* pupil_xy, int32_t n_rays, double* xy_out, int32_t* ngood_out,
                                     void* stream)
{
    return trace_field_points_run(optics_dev ? &optics_dev->optics : nullptr, true, thx, thy, n, wave_nm, pupil_xy, n_rays, xy_out,
                                  ngood_out, stream);
}

}  // extern "C"
