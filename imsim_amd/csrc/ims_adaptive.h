// ims_adaptive.h -- section of the one translation unit (imsim_hip.hip): adaptive moments of the delivered PSF, iterated on the device.
//
// The rows are field points, as for ims_psf_moments.  Photon k of a row is the photon k_psf_moments makes for it -- shoot / run_psf /
// run_ops on the same Philox counters -- and (dx, dy) is k_psf_moments' offset.  Nothing of the photon is stored: every round shoots
// the row's photons again and reduces them under the row's current elliptical Gaussian weight (Bernstein & Jarvis 2002; Hirata &
// Seljak 2003), then one thread moves the weight towards the profile.  Per row the state is the centre (x0, y0) and the weight
// matrix (Mxx, Mxy, Myy), in the units of the stage.
//
// Pass (k_psf_adaptive_pass), per photon with w = flux != 0:
//   u = dx - x0, v = dy - y0, det = Mxx Myy - Mxy^2, rho2 = (Myy u u - 2 Mxy u v + Mxx v v) / det, g = w dexp(-rho2 / 2)
//   A = sum g; Bx, By = sum g u, g v; Cxx, Cxy, Cyy = sum g u u, g u v, g v v; R = sum g rho2^2; W = sum w; the counts used, dropped
// reduced as moments_block_sum reduces: the xor butterfly over the wavefront, the four wavefronts in turn through LDS, one record of
// AD_N doubles per 256-photon segment.  No atomics.
// Update (k_psf_adaptive_update), one workgroup per row: the row's records are added in k_psf_moments_combine's order, then thread 0
// evaluates, in f64 and in this order,
//   T = Mxx + Myy, D = sqrt((Mxx - Myy)^2 + 4 Mxy^2), a2 = (T + D) / 2, b2 = (T - D) / 2, s = sqrt(b2)
//   ex = 2 Bx / (A s), ey = 2 By / (A s), exx = 4 (Cxx / A - Mxx / 2) / b2, exy and eyy likewise, each clipped to [-1/4, 1/4]
//   conv = max |e.| sqrt(a2 / b2);  x0 += ex s, y0 += ey s, Mxx += exx b2, Mxy += exy b2, Myy += eyy b2;  iter += 1
// Status of a row (int32): 0 converged (conv < tol after the update), 1 running, 2 failed (A not finite or <= 0, or the new matrix not
// finite or not positive definite: the state stays at its last valid values), 3 no photon arrived (the state is NaN).  Only a row
// of status 1 is worked on: the workgroups of a frozen row return before they shoot a photon, and its state, status, iter and rho4
// are left alone.  A row's result depends on nothing but the row.
//
// Kernels: k_psf_adaptive_pass<CHAIN, PSF, LAYOUT>, the variants of k_psf_moments; k_psf_adaptive_update.  Entry point: ims_psf_adaptive.
#pragma once

constexpr int AD_N = 10;           // A, Bx, By, Cxx, Cxy, Cyy, R, sum w, photons used, photons dropped (counts as exact f64 integers)
constexpr int AD_RUNNING = 1, AD_CONVERGED = 0, AD_FAILED = 2, AD_EMPTY = 3;

// the workgroup's totals: thread q < AD_N returns total q, the others 0 (moments_block_sum's order of additions)
__device__ __forceinline__ double adaptive_block_sum(double (&v)[AD_N])
{
    __shared__ double part[4][AD_N];
#pragma unroll
    for (int q = 0; q < AD_N; ++q) v[q] = wave_sum(v[q]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < AD_N; ++q) part[threadIdx.x >> 6][q] = v[q];
    }
    __syncthreads();
    const int q = (int)threadIdx.x;
    return q < AD_N ? ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q] : 0.0;
}

template <int CHAIN, int PSF, unsigned long long LAYOUT>
__global__ __launch_bounds__(256, IMS_FUSED_WAVES) void k_psf_adaptive_pass(const ims_render_params_t P, const int stage,
                                                                            const double* __restrict__ state,
                                                                            const int32_t* __restrict__ status,
                                                                            double* __restrict__ partial)
{
    const int64_t per = (P.n_segments + N_XCD - 1) / N_XCD;
    const int64_t b = blockIdx.x;
    if ((b / N_XCD) >= per) return;
    const int64_t seg = xcd_segment(b, P.n_segments);
    if (seg >= P.n_segments) return;
    const int64_t oi = P.seg_object ? (int64_t)P.seg_object[seg] : find_object(P.seg_prefix, P.n_objects, seg);
    // (uniform over the workgroup: a frozen row costs its workgroups this one load, and no barrier has been reached yet)
    if (status[2 * oi] != AD_RUNNING) return;
    const ims_object_t& o = P.objects[oi];
    if constexpr (PSF >= 3) optical_setup(P, o);     // the row's optical phase screen, by all 256 threads (ims_optical.h)
    const double x0 = state[5 * oi], y0 = state[5 * oi + 1], mxx = state[5 * oi + 2], mxy = state[5 * oi + 3], myy = state[5 * oi + 4];
    const double det = mxx * myy - mxy * mxy;
    const int64_t j = (seg - P.seg_prefix[oi]) * P.seg_size + threadIdx.x;
    double v[AD_N] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    // (the lanes past the row's last photon stay: they hold the zeros of the sums)
    if (j < o.n_phot) {
        const int64_t k = o.phot_first + j;
        Photon ph;
        Rng rng;
        rng_reset(rng);
        shoot(P, o, k, rng, ph);
        run_psf<PSF>(P, o, k, rng, ph);
        double dx = ph.x, dy = ph.y;
        if (stage == 2) {
            ph.x = o.x0 + ph.x;
            ph.y = o.y0 + ph.y;
            run_ops<CHAIN, LAYOUT>(P, o, k, rng, ph);
            dx = ph.x - o.x0; dy = ph.y - o.y0;
        }
        if (ph.flux != 0.0) {
            const double w = ph.flux, du = dx - x0, dv = dy - y0;
            const double rho2 = (myy * du * du - 2.0 * mxy * du * dv + mxx * dv * dv) / det;
            const double g = w * dexp(-0.5 * rho2);
            const double gu = g * du, gv = g * dv;
            v[0] = g; v[1] = gu; v[2] = gv; v[3] = gu * du; v[4] = gu * dv; v[5] = gv * dv; v[6] = g * rho2 * rho2;
            v[7] = w; v[8] = 1.0;
        } else v[9] = 1.0;
    }
    const double tot = adaptive_block_sum(v);
    if (threadIdx.x < AD_N) partial[seg * AD_N + threadIdx.x] = tot;
}

__device__ __forceinline__ double adaptive_clip(double e)       // (a NaN stays a NaN)
{
    return e < -0.25 ? -0.25 : (e > 0.25 ? 0.25 : e);
}

__global__ __launch_bounds__(256) void k_psf_adaptive_update(const int64_t* __restrict__ seg_prefix, const double* __restrict__ partial,
                                                             const double tol, double* __restrict__ state,
                                                             int32_t* __restrict__ status, double* __restrict__ aux)
{
    __shared__ double tot[AD_N];
    const int64_t oi = blockIdx.x;
    if (status[2 * oi] != AD_RUNNING) return;        // uniform: a frozen row is left alone
    const int64_t s0 = seg_prefix[oi], s1 = seg_prefix[oi + 1];
    double v[AD_N] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int64_t s = s0 + threadIdx.x; s < s1; s += 256) {
#pragma unroll
        for (int q = 0; q < AD_N; ++q) v[q] = v[q] + partial[s * AD_N + q];
    }
    const double t = adaptive_block_sum(v);
    if (threadIdx.x < AD_N) tot[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double A = tot[0], Bx = tot[1], By = tot[2], Cxx = tot[3], Cxy = tot[4], Cyy = tot[5], R = tot[6];
    double* st = state + 5 * oi;
    double* ax = aux + 4 * oi;
    ax[1] = tot[7]; ax[2] = tot[8]; ax[3] = tot[9];
    if (tot[8] == 0.0) {                             // no photon arrived
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        st[0] = nan; st[1] = nan; st[2] = nan; st[3] = nan; st[4] = nan; ax[0] = nan;
        status[2 * oi] = AD_EMPTY;
        return;
    }
    if (!(A > 0.0) || !isfinite(A)) { status[2 * oi] = AD_FAILED; return; }
    const double mxx = st[2], mxy = st[3], myy = st[4];
    const double T = mxx + myy;
    const double D = sqrt((mxx - myy) * (mxx - myy) + 4.0 * mxy * mxy);
    const double a2 = (T + D) / 2.0, b2 = (T - D) / 2.0, s = sqrt(b2);
    const double ex = adaptive_clip(2.0 * Bx / (A * s)), ey = adaptive_clip(2.0 * By / (A * s));
    const double exx = adaptive_clip(4.0 * (Cxx / A - mxx / 2.0) / b2);
    const double exy = adaptive_clip(4.0 * (Cxy / A - mxy / 2.0) / b2);
    const double eyy = adaptive_clip(4.0 * (Cyy / A - myy / 2.0) / b2);
    double big = fabs(ex);
    if (fabs(ey) > big) big = fabs(ey);
    if (fabs(exx) > big) big = fabs(exx);
    if (fabs(exy) > big) big = fabs(exy);
    if (fabs(eyy) > big) big = fabs(eyy);
    const double conv = big * sqrt(a2 / b2);
    const double nxx = mxx + exx * b2, nxy = mxy + exy * b2, nyy = myy + eyy * b2;
    const double ndet = nxx * nyy - nxy * nxy;
    if (!isfinite(nxx) || !isfinite(nxy) || !isfinite(nyy) || !(nxx > 0.0) || !(ndet > 0.0)) { status[2 * oi] = AD_FAILED; return; }
    st[0] = st[0] + ex * s; st[1] = st[1] + ey * s; st[2] = nxx; st[3] = nxy; st[4] = nyy;
    ax[0] = R / A;
    status[2 * oi + 1] = status[2 * oi + 1] + 1;
    if (conv < tol) status[2 * oi] = AD_CONVERGED;
}

extern "C" {

int ims_psf_adaptive(const ims_render_params_t* params, int32_t stage, int32_t n_rounds, double tol, double* partial_dev,
                     double* state_dev, int32_t* status_dev, double* aux_dev, void* stream)
{
    int rc = check_params(params);
    if (rc) return rc;
    if (stage != 1 && stage != 2) return set_err(IMS_ERR_ARG, "psf_adaptive: stage must be 1 (shoot + PSF) or 2 (+ photon operators)");
    if (n_rounds < 1) return set_err(IMS_ERR_ARG, "psf_adaptive: n_rounds must be at least 1");
    if (!(tol > 0.0) || !std::isfinite(tol)) return set_err(IMS_ERR_ARG, "psf_adaptive: tol must be positive and finite");
    if (params->n_objects == 0) return IMS_OK;
    if (!state_dev || !status_dev || !aux_dev) return set_err(IMS_ERR_ARG, "psf_adaptive: state / status / aux is NULL");
    if (params->n_segments > 0 && !partial_dev) return set_err(IMS_ERR_ARG, "psf_adaptive: partial is NULL");
    if (params->n_objects > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "psf_adaptive: too many points for one call");
    // (the grid of the pass is the segment count rounded up to a multiple of the XCDs)
    if (params->n_segments > 0x7fffffffLL - N_XCD) return set_err(IMS_ERR_ARG, "psf_adaptive: too many segments for one call");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_for_segments(params->n_segments));
    const unsigned lds = photon_lds_pad(params);
    for (int32_t round = 0; round < n_rounds; ++round) {
        if (params->n_segments > 0) {
            rc = launch_photon_variant<1>(select_photon_variant(params, 1), [&](auto k) {
                using K = decltype(k);
                hipLaunchKernelGGL((k_psf_adaptive_pass<K::chain, K::psf, K::layout>), grid, dim3(256), lds, st, *params, (int)stage,
                                   (const double*)state_dev, (const int32_t*)status_dev, partial_dev);
            });
            if (rc) return rc;
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_psf_adaptive_update, dim3((unsigned)params->n_objects), dim3(256), 0, st, params->seg_prefix,
                           (const double*)partial_dev, tol, state_dev, status_dev, aux_dev);
        HIP_TRY(hipGetLastError());
    }
    return IMS_OK;
}

}  // extern "C"
