// ims_psf_image.h -- section of the one translation unit (imsim_hip.hip): postage stamps of the delivered PSF, up to the sensor.
//
// The rows are field points, as for ims_psf_moments and ims_psf_profile.  Photon k of a row is the photon k_psf_moments,
// k_psf_profile and k_shoot_photons make for it -- shoot / run_psf / run_ops on the same Philox counters.  Nothing of the photon
// is stored: it adds one to a cell of the row's [ny][nx] stamp of counts, to the row's `outside` count, or to its `dropped` count.
//
// Stages: 1 the offset after the PSF components [arcsec]; 2 ph.x - o.x0, ph.y - o.y0 after the operator chain [pixels]; 3 as 2,
// then land_convert (ims_photon.h: conversion depth from the absorption length, lateral walk of an inclined ray down to it,
// diffusion) and x0 - o.x0, y0 - o.y0 of the converted position [pixels].  Stage 3 converts the rows k_shoot_photons<2> converts
// (a Silicon sensor, the row not IMS_OBJ_FAINT) with the has_angles that kernel passes, so its offsets are the converted pool's bit
// for bit; land_convert draws SLOT_SENSOR only, so stages 1 and 2 of a row are the same photons.  A photon land_convert loses
// (zconv < 0) is dropped, as a photon of flux 0 is.
// What stage 3 is NOT: there is no pixel search (land_search).  The stamp bins continuous positions on a regular grid; tree rings
// and brighter-fatter move pixel boundaries, not photons, and cannot appear in it.
//
// Binning (f64 products, sums and comparisons only; the file is built without contraction, so numpy restates it bit for bit):
//   u = dx * inv_scale + nx / 2, v = dy * inv_scale + ny / 2; 0 <= u < nx and 0 <= v < ny: cell (floor u, floor v); anything
//   else (beside the stamp, a NaN): the row's `outside`.  The host passes inv_scale: no division here.
//
// A workgroup walks a run of consecutive 256-photon segments.  Almost every photon of a PSF lands in a few hundred cells around
// the centre, so the workgroup keeps a u32 window of at most 64 x 64 cells, centred on the stamp, in LDS (16 KB: the footprint
// of k_psf_profile's histogram, so photon_lds_pad and IMS_FUSED_WAVES leave the residency of the photon kernels as it is) and
// adds to it with LDS integer atomics; when the row changes or the run ends the non-zero cells go to the row's int64 stamp with
// 64-bit global atomics, thread t the cells t, t + 256, ... (consecutive addresses along a window row).  A stamp of at most
// 64 x 64 is all window.  Cells of a larger stamp outside the window (the 1/r^2 halo, the spikes) take their photons straight to
// global memory, one 64-bit atomic each, as ims_fft_reshoot's 16 x 16 window does.  A run holds fewer than 2^32 photons, so no
// u32 cell overflows.  All sums are integer: the result does not depend on the run length, the order of arrival, or the other
// rows of the call.
// The window's rows are 64 cells apart: photons of one column of the core share an LDS bank, and equal cells serialise in the
// atomic unit anyway.  Neither is padded away: a photon costs one LDS atomic against the thousands of VALU cycles of its trace.
//
// Kernel: k_psf_image<CHAIN, PSF, LAYOUT>, the variants of k_psf_moments.  Entry point: ims_psf_image.
#pragma once

constexpr int IMG_WIN = 64;                                          // the LDS window is at most IMG_WIN x IMG_WIN cells
constexpr unsigned IMG_LDS_BYTES = IMG_WIN * IMG_WIN * 4 + 8;

template <int CHAIN, int PSF, unsigned long long LAYOUT>
__global__ __launch_bounds__(256, IMS_FUSED_WAVES) void k_psf_image(const ims_render_params_t P, const int stage, const ims_psf_image_t S,
                                                                    const double* __restrict__ centre, const int64_t run,
                                                                    int64_t* __restrict__ counts, int64_t* __restrict__ outside,
                                                                    int64_t* __restrict__ dropped)
{
    __shared__ unsigned int win[IMG_WIN * IMG_WIN];
    __shared__ unsigned int lost, beside;
    const int nx = S.nx, ny = S.ny;
    const int wx = nx < IMG_WIN ? nx : IMG_WIN, wy = ny < IMG_WIN ? ny : IMG_WIN;       // the window, centred on the stamp
    const int wx0 = (nx - wx) >> 1, wy0 = (ny - wy) >> 1;
    const int n_win = wy * IMG_WIN;                                  // window cell c = (row c >> 6, column c & 63), columns < wx used
    const int64_t n_cells = (int64_t)nx * ny;
    const double inv_scale = S.inv_scale, half_x = 0.5 * (double)nx, half_y = 0.5 * (double)ny, lim_x = (double)nx, lim_y = (double)ny;
    const int tid = (int)threadIdx.x;
    for (int t = tid; t < n_win; t += 256) win[t] = 0u;
    if (tid == 0) { lost = 0u; beside = 0u; }
    const bool convert = stage == 3 && P.sensor != nullptr && P.sensor->kind == IMS_SENSOR_SILICON;
    const bool has_angles = (CHAIN == 1) ? true : chain_has_angles(P);       // as k_shoot_photons<2> passes it to land_convert
    const int64_t s0 = (int64_t)blockIdx.x * run;
    const int64_t s1 = (s0 + run < P.n_segments) ? s0 + run : P.n_segments;
    int64_t row = -1;                                                // the row the window holds photons of
    unsigned int n_lost = 0u, n_beside = 0u;                         // this thread's dropped / outside photons of that row
    // (every branch on s, oi and row is uniform over the workgroup: the barriers below are reached by all 256 threads)
    for (int64_t s = s0; s < s1; ++s) {
        const int64_t oi = P.seg_object ? (int64_t)P.seg_object[s] : find_object(P.seg_prefix, P.n_objects, s);
        if (oi != row) {
            if (n_lost) atomicAdd(&lost, n_lost);
            if (n_beside) atomicAdd(&beside, n_beside);
            n_lost = 0u; n_beside = 0u;
            __syncthreads();                                         // the adds of the row before (and the zeroing) are done
            if (row >= 0) {
                int64_t* stamp = counts + row * n_cells + (int64_t)wy0 * nx + wx0;
                for (int t = tid; t < n_win; t += 256) {
                    const unsigned int c = win[t];
                    if (c) { atomicAdd((unsigned long long*)(stamp + (int64_t)(t >> 6) * nx + (t & 63)), (unsigned long long)c); win[t] = 0u; }
                }
                if (tid == 0 && lost) { atomicAdd((unsigned long long*)(dropped + row), (unsigned long long)lost); lost = 0u; }
                if (tid == 0 && beside) { atomicAdd((unsigned long long*)(outside + row), (unsigned long long)beside); beside = 0u; }
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
        if (stage >= 2) {
            ph.x = o.x0 + ph.x;
            ph.y = o.y0 + ph.y;
            run_ops<CHAIN, LAYOUT>(P, o, k, rng, ph);
            dx = ph.x - o.x0; dy = ph.y - o.y0;
        }
        if (ph.flux == 0.0) { ++n_lost; continue; }
        if (convert && !(o.flags & IMS_OBJ_FAINT)) {
            double x0, y0, zconv;
            bool coin;
            if (!land_convert(P, o, k, rng, ph, has_angles, x0, y0, zconv, coin)) { ++n_lost; continue; }
            dx = x0 - o.x0; dy = y0 - o.y0;
        }
        if (centre != nullptr) { dx = dx - centre[2 * oi]; dy = dy - centre[2 * oi + 1]; }
        const double u = dx * inv_scale + half_x, v = dy * inv_scale + half_y;
        if (!(u >= 0.0 && u < lim_x && v >= 0.0 && v < lim_y)) { ++n_beside; continue; }       // (a NaN fails every comparison)
        const int ix = (int)u, iy = (int)v;                          // floor: u, v are not negative; 0 <= ix < nx, 0 <= iy < ny
        const int cx = ix - wx0, cy = iy - wy0;
        if ((unsigned)cx < (unsigned)wx && (unsigned)cy < (unsigned)wy) atomicAdd(&win[cy * IMG_WIN + cx], 1u);
        else atomicAdd((unsigned long long*)(counts + oi * n_cells + (int64_t)iy * nx + ix), 1ull);
    }
    if (row < 0) return;
    if (n_lost) atomicAdd(&lost, n_lost);
    if (n_beside) atomicAdd(&beside, n_beside);
    __syncthreads();
    int64_t* stamp = counts + row * n_cells + (int64_t)wy0 * nx + wx0;
    for (int t = tid; t < n_win; t += 256) {
        const unsigned int c = win[t];
        if (c) atomicAdd((unsigned long long*)(stamp + (int64_t)(t >> 6) * nx + (t & 63)), (unsigned long long)c);
    }
    if (tid == 0 && lost) atomicAdd((unsigned long long*)(dropped + row), (unsigned long long)lost);
    if (tid == 0 && beside) atomicAdd((unsigned long long*)(outside + row), (unsigned long long)beside);
}

extern "C" {

int ims_psf_image(const ims_render_params_t* params, int32_t stage, const ims_psf_image_t* spec, const double* centre_dev,
                  int64_t* counts_dev, int64_t* outside_dev, int64_t* dropped_dev, void* stream)
{
    if (!spec) return set_err(IMS_ERR_ARG, "psf_image: spec is NULL");
    int rc = check_params(params);
    if (rc) return rc;
    if (stage < 1 || stage > 3)
        return set_err(IMS_ERR_ARG, "psf_image: stage must be 1 (shoot + PSF), 2 (+ photon operators) or 3 (+ conversion in the sensor)");
    if (stage == 3 && !params->sensor) return set_err(IMS_ERR_ARG, "psf_image: stage 3 needs params->sensor, which is NULL");
    if (spec->nx < 1 || spec->nx > IMS_PSF_IMAGE_MAX) return set_err(IMS_ERR_ARG, "psf_image: nx must be 1 .. 512");
    if (spec->ny < 1 || spec->ny > IMS_PSF_IMAGE_MAX) return set_err(IMS_ERR_ARG, "psf_image: ny must be 1 .. 512");
    if (!(spec->inv_scale > 0.0) || !std::isfinite(spec->inv_scale)) return set_err(IMS_ERR_ARG, "psf_image: inv_scale must be finite and positive");
    if (stage >= 2)
        for (int q = 0; q < params->n_ops; ++q)
            if (params->ops[q].kind == IMS_OP_BANDPASS_RATIO)
                return set_err(IMS_ERR_UNSUPPORTED, "psf_image: the chain holds a BandpassRatio operator (photons of unequal flux; the counts are unweighted)");
    if (params->n_objects == 0) return IMS_OK;
    if (!counts_dev || !outside_dev || !dropped_dev) return set_err(IMS_ERR_ARG, "psf_image: counts / outside / dropped is NULL");
    if (params->n_objects > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "psf_image: too many points for one call");
    hipStream_t st = (hipStream_t)stream;
    const size_t n_cells = (size_t)spec->nx * (size_t)spec->ny;
    HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)params->n_objects * n_cells * sizeof(int64_t), st));
    HIP_TRY(hipMemsetAsync(outside_dev, 0, (size_t)params->n_objects * sizeof(int64_t), st));
    HIP_TRY(hipMemsetAsync(dropped_dev, 0, (size_t)params->n_objects * sizeof(int64_t), st));
    if (params->n_segments == 0) return IMS_OK;
    // a run of 2^23 segments is 2^31 photons: the u32 cells of a workgroup's window cannot overflow (ims_psf_profile's cap)
    int64_t run = (params->n_segments + PROF_TARGET_RUNS - 1) / PROF_TARGET_RUNS;
    if (run > ((int64_t)1 << 23)) run = (int64_t)1 << 23;
    const int64_t n_runs = (params->n_segments + run - 1) / run;
    if (n_runs > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "psf_image: too many photons for one call");
    // the dynamic LDS the photon kernels ask for to hold their residency (photon_lds_pad), less what the window takes itself
    const unsigned pad = photon_lds_pad(params), lds = pad > IMG_LDS_BYTES ? pad - IMG_LDS_BYTES : 0u;
    rc = launch_photon_variant<1>(select_photon_variant(params, 1), [&](auto k) {
        using K = decltype(k);
        hipLaunchKernelGGL((k_psf_image<K::chain, K::psf, K::layout>), dim3((unsigned)n_runs), dim3(256), lds, st, *params, (int)stage, *spec,
                           centre_dev, run, counts_dev, outside_dev, dropped_dev);
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

}  // extern "C"
