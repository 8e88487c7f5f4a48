// ims_profile.h -- section of the one translation unit (imsim_hip.hip): radial and azimuthal histograms of the delivered PSF.
//
// The rows are field points, as for ims_psf_moments.  Photon k of a row is the photon k_psf_moments and k_shoot_photons make for it
// -- shoot / run_psf / run_ops on the same Philox counters -- and (dx, dy) is k_psf_moments' offset, less the row's centre when one
// is given.  Nothing of the photon is stored: it adds one to a bin of the row's [n_r + 2][n_phi + 1] table of counts.
//
// Binning (f64 products, sums and comparisons only; the file is built without contraction, so numpy restates it bit for bit):
//   r2 = dx * dx + dy * dy; radial index = the number of edges e <= r2 (0 underflow, 1 .. n_r the bins, n_r + 1 overflow);
//   t_b = c_b * dy - s_b * dx; sector index = the first b with t_b >= 0 and t_{b + 1} < 0 (b + 1 wrapping to 0), n_phi when
//   there is none (the centre, a rounding gap, a NaN); n_phi = 0 has the one column.
//
// A workgroup walks a run of consecutive 256-photon segments.  Its histogram is u32 in LDS (17 160 bytes at 66 x 65), added to
// with LDS integer atomics, with the edges and directions staged beside it once; when the row changes or the run ends the non-zero
// bins go to the row's int64 counts with 64-bit global atomics, thread t the bins t, t + 256, ... (consecutive addresses).  A run
// holds fewer than 2^32 photons, so no bin overflows.  All sums are integer: the result does not depend on the run length, the
// order of arrival, or the other rows of the call.
//
// Kernel: k_psf_profile<CHAIN, PSF, LAYOUT>, the variants of k_psf_moments.  Entry point: ims_psf_profile.
#pragma once

constexpr int PROF_MAX_R = 64, PROF_MAX_PHI = 64;
constexpr int PROF_MAX_BINS = (PROF_MAX_R + 2) * (PROF_MAX_PHI + 1);
constexpr unsigned PROF_LDS_BYTES = PROF_MAX_BINS * 4 + (PROF_MAX_R + 1) * 8 + PROF_MAX_PHI * 16 + 4;
// runs per launch the host aims at: two rounds of four workgroups on each of 256 CUs
constexpr int64_t PROF_TARGET_RUNS = 2048;

template <int CHAIN, int PSF, unsigned long long LAYOUT>
__global__ __launch_bounds__(256, IMS_FUSED_WAVES) void k_psf_profile(const ims_render_params_t P, const int stage, const ims_psf_profile_t S,
                                                                      const double* __restrict__ centre, const int64_t run,
                                                                      int64_t* __restrict__ counts, int64_t* __restrict__ dropped)
{
    __shared__ unsigned int hist[PROF_MAX_BINS];
    __shared__ double edge[PROF_MAX_R + 1];
    __shared__ double dir[2 * PROF_MAX_PHI];
    __shared__ unsigned int lost;
    const int n_edge = S.n_r + 1, n_phi = S.n_phi, n_col = S.n_phi + 1, n_bins = (S.n_r + 2) * n_col;
    const int tid = (int)threadIdx.x;
    for (int t = tid; t < n_bins; t += 256) hist[t] = 0u;
    for (int t = tid; t < n_edge; t += 256) edge[t] = S.r2_edge_dev[t];
    for (int t = tid; t < 2 * n_phi; t += 256) dir[t] = S.dir_dev[t];
    if (tid == 0) lost = 0u;
    const int64_t s0 = (int64_t)blockIdx.x * run;
    const int64_t s1 = (s0 + run < P.n_segments) ? s0 + run : P.n_segments;
    int64_t row = -1;                                                // the row the histogram holds photons of
    unsigned int n_lost = 0u;                                        // this thread's dropped photons of that row
    // (every branch on s, oi and row is uniform over the workgroup: the barriers below are reached by all 256 threads)
    for (int64_t s = s0; s < s1; ++s) {
        const int64_t oi = P.seg_object ? (int64_t)P.seg_object[s] : find_object(P.seg_prefix, P.n_objects, s);
        if (oi != row) {
            if (n_lost) atomicAdd(&lost, n_lost);
            n_lost = 0u;
            __syncthreads();                                         // the adds of the row before (and the staging) are done
            if (row >= 0) {
                for (int t = tid; t < n_bins; t += 256) {
                    const unsigned int c = hist[t];
                    if (c) { atomicAdd((unsigned long long*)(counts + row * n_bins + t), (unsigned long long)c); hist[t] = 0u; }
                }
                if (tid == 0 && lost) { atomicAdd((unsigned long long*)(dropped + row), (unsigned long long)lost); lost = 0u; }
            }
            row = oi;
            if constexpr (PSF >= 3) optical_setup(P, P.objects[oi]);     // the row's optical phase screen (ims_optical.h)
            __syncthreads();
        }
        const ims_object_t& o = P.objects[oi];
        const int64_t j = (s - P.seg_prefix[oi]) * P.seg_size + tid;
        if (j >= o.n_phot) continue;
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
        if (ph.flux == 0.0) { ++n_lost; continue; }
        if (centre != nullptr) { dx = dx - centre[2 * oi]; dy = dy - centre[2 * oi + 1]; }
        const double r2 = dx * dx + dy * dy;
        int lo = 0, hi = n_edge;                                     // the number of edges <= r2 (a NaN is below every edge)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (edge[mid] <= r2) lo = mid + 1; else hi = mid;
        }
        int sector = n_phi;
        if (n_phi > 0) {
            const double t0 = dir[0] * dy - dir[1] * dx;
            double here = t0;
            for (int b = 0; b < n_phi; ++b) {
                const double next = (b + 1 < n_phi) ? dir[2 * b + 2] * dy - dir[2 * b + 3] * dx : t0;
                if (here >= 0.0 && next < 0.0) { sector = b; break; }
                here = next;
            }
        }
        atomicAdd(&hist[lo * n_col + sector], 1u);
    }
    if (row < 0) return;
    if (n_lost) atomicAdd(&lost, n_lost);
    __syncthreads();
    for (int t = tid; t < n_bins; t += 256) {
        const unsigned int c = hist[t];
        if (c) atomicAdd((unsigned long long*)(counts + row * n_bins + t), (unsigned long long)c);
    }
    if (tid == 0 && lost) atomicAdd((unsigned long long*)(dropped + row), (unsigned long long)lost);
}

extern "C" {

int ims_psf_profile(const ims_render_params_t* params, int32_t stage, const ims_psf_profile_t* spec, const double* centre_dev,
                    int64_t* counts_dev, int64_t* dropped_dev, void* stream)
{
    if (!spec) return set_err(IMS_ERR_ARG, "psf_profile: spec is NULL");
    int rc = check_params(params);
    if (rc) return rc;
    if (stage != 1 && stage != 2) return set_err(IMS_ERR_ARG, "psf_profile: stage must be 1 (shoot + PSF) or 2 (+ photon operators)");
    if (spec->n_r < 1 || spec->n_r > PROF_MAX_R) return set_err(IMS_ERR_ARG, "psf_profile: n_r must be 1 .. 64");
    if (spec->n_phi != 0 && (spec->n_phi < 3 || spec->n_phi > PROF_MAX_PHI)) return set_err(IMS_ERR_ARG, "psf_profile: n_phi must be 0 or 3 .. 64");
    if (params->n_objects == 0) return IMS_OK;
    if (!counts_dev || !dropped_dev) return set_err(IMS_ERR_ARG, "psf_profile: counts / dropped is NULL");
    if (!spec->r2_edge_dev) return set_err(IMS_ERR_ARG, "psf_profile: r2_edge is NULL");
    if (spec->n_phi > 0 && !spec->dir_dev) return set_err(IMS_ERR_ARG, "psf_profile: dir is NULL");
    if (params->n_objects > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "psf_profile: too many points for one call");
    if (stage == 2)
        for (int q = 0; q < params->n_ops; ++q)
            if (params->ops[q].kind == IMS_OP_BANDPASS_RATIO)
                return set_err(IMS_ERR_UNSUPPORTED, "psf_profile: the chain holds a BandpassRatio operator (photons of unequal flux; the counts are unweighted)");
    hipStream_t st = (hipStream_t)stream;
    const size_t n_bins = (size_t)(spec->n_r + 2) * (size_t)(spec->n_phi + 1);
    HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)params->n_objects * n_bins * sizeof(int64_t), st));
    HIP_TRY(hipMemsetAsync(dropped_dev, 0, (size_t)params->n_objects * sizeof(int64_t), st));
    if (params->n_segments == 0) return IMS_OK;
    // a run of 2^23 segments is 2^31 photons: the u32 bins of a workgroup cannot overflow
    int64_t run = (params->n_segments + PROF_TARGET_RUNS - 1) / PROF_TARGET_RUNS;
    if (run > ((int64_t)1 << 23)) run = (int64_t)1 << 23;
    const int64_t n_runs = (params->n_segments + run - 1) / run;
    if (n_runs > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "psf_profile: too many photons for one call");
    // the dynamic LDS the photon kernels ask for to hold their residency (photon_lds_pad), less what the histogram takes itself
    const unsigned pad = photon_lds_pad(params), lds = pad > PROF_LDS_BYTES ? pad - PROF_LDS_BYTES : 0u;
    rc = launch_photon_variant<1>(select_photon_variant(params, 1), [&](auto k) {
        using K = decltype(k);
        hipLaunchKernelGGL((k_psf_profile<K::chain, K::psf, K::layout>), dim3((unsigned)n_runs), dim3(256), lds, st, *params, (int)stage, *spec,
                           centre_dev, run, counts_dev, dropped_dev);
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

}  // extern "C"
