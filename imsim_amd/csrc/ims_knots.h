// ims_knots.h -- section of the one translation unit (imsim_hip.hip): RandomKnots on the FFT branch.
//
// A knots object is N delta functions of equal flux (shoot(), ims_photon.h): its spectrum is the point source's times the structure
// factor S(k) = (1 / N) sum_m exp(-i k . d_m), d_m the knot's displacement in arcsec along the pixel axes.  ims_fft_kspace_fill fills
// such an object as a point (prof_ktable IMS_PROF_POINT); the pass here multiplies its half spectrum by S before the inverse transform.
// Base band only (ims_fft_params_t.n_alias == 0): S at k + a ks is not a common factor of a folded sum.
//
// Kernels: k_knot_positions, k_fft_knots_factor.
// Entry points: ims_knot_positions, ims_fft_knots_factor.
#pragma once

// d_m of every knot of every FFT row with knots: the calls of shoot()'s knots arm in its order, then jac' (build_fft_objects:
// pixel_scale x winv x jac) in place of jac and winv.  One workgroup per row.
__global__ __launch_bounds__(256) void k_knot_positions(uint64_t seed, const ims_fft_object_t* __restrict__ objs, const int32_t* __restrict__ n_knots,
                                                        const double* __restrict__ sigma, const int64_t* __restrict__ knot_offset,
                                                        double* __restrict__ knot_xy)
{
    const int64_t oi = blockIdx.x;
    const int32_t n = n_knots[oi];
    if (n <= 0) return;
    const ims_fft_object_t& o = objs[oi];
    const double sg = sigma[oi];
    const int64_t at = knot_offset[oi];
    for (int32_t m = (int32_t)threadIdx.x; m < n; m += 256) {
        Rng kr;
        rng_reset(kr);
        rng_block(kr, seed, o.obj_id, (int64_t)m, SLOT_KNOT);
        double g0, g1;
        gauss_words(kr.w[0], kr.w[1], g0, g1);
        const double gu = sg * g0, gv = sg * g1;
        knot_xy[2 * (at + m)] = o.jac[0] * gu + o.jac[1] * gv;
        knot_xy[2 * (at + m) + 1] = o.jac[2] * gu + o.jac[3] * gv;
    }
}

// The structure-factor pass.  A workgroup owns KNOT_ROWS x KNOT_COLS points of ONE object's half spectrum (blockIdx.z: the object's
// place in the list of rows with knots; tiles beyond the object's own grid leave at once -- the launch is sized for the largest grid).
// Knots come in chunks of KNOT_CHUNK: the workgroup forms exp(-i kx_j dx_m) for the tile's columns and exp(-i ky_i dy_m) for its rows
// ONCE each into LDS (one dsincos per (knot, column) and per (knot, row)), then every thread accumulates the complex products of its
// column with KNOT_ROWS / 4 rows in registers: per knot a (rows x 1) . (1 x columns) update, over the knots the complex
// (rows x N) . (N x columns) product.
// LDS: cosines and sines apart, [knot][column]: the 64 lanes of a wavefront read 64 consecutive doubles (ds_read_b64: two halves of 32
// lanes x 8 B = one 256-B bank row each, no conflict); the row phases are read at a wave-uniform address (a broadcast).  48 KB per
// workgroup: three workgroups on a CU's 160 KB.
// The sum of a point runs over m ascending with one association, whatever the tile or the chunk: the result does not depend on the
// launch geometry.  Cosine 1 and sine 0 at k = 0 are exact, so S(0, 0) = N / N = 1.
constexpr int KNOT_ROWS = 32, KNOT_COLS = 64, KNOT_CHUNK = 32, KNOT_PER_THREAD = KNOT_ROWS / 4;
__global__ __launch_bounds__(256) void k_fft_knots_factor(const ims_fft_params_t P, const ims_fft_object_t* __restrict__ objs,
                                                          const int32_t* __restrict__ knot_rows, const int32_t* __restrict__ n_knots,
                                                          const int64_t* __restrict__ knot_offset, const double* __restrict__ knot_xy,
                                                          double* __restrict__ kbuf)
{
    __shared__ double col_c[KNOT_CHUNK * KNOT_COLS], col_s[KNOT_CHUNK * KNOT_COLS];
    __shared__ double row_c[KNOT_CHUNK * KNOT_ROWS], row_s[KNOT_CHUNK * KNOT_ROWS];
    const int32_t oi = knot_rows[blockIdx.z];
    const ims_fft_object_t& o = objs[oi];
    const int n = o.nfft, nh = n / 2 + 1;
    const int j0 = (int)blockIdx.x * KNOT_COLS, i0 = (int)blockIdx.y * KNOT_ROWS;
    const int32_t N = n_knots[oi];
    if (j0 >= nh || i0 >= n || N <= 0) return;                       // (uniform over the workgroup)
    const double* __restrict__ xy = knot_xy + 2 * knot_offset[oi];
    const double dk = TWO_PI / ((double)n * P.pixel_scale);
    const int lane = (int)(threadIdx.x & 63u);
    const int r0 = (int)(threadIdx.x >> 6) * KNOT_PER_THREAD;        // first of this wavefront's rows inside the tile
    double acc_re[KNOT_PER_THREAD], acc_im[KNOT_PER_THREAD];
#pragma unroll
    for (int r = 0; r < KNOT_PER_THREAD; ++r) { acc_re[r] = 0.0; acc_im[r] = 0.0; }
    for (int32_t m0 = 0; m0 < N; m0 += KNOT_CHUNK) {
        const int nm = (N - m0 < KNOT_CHUNK) ? (int)(N - m0) : KNOT_CHUNK;
        if (m0 > 0) __syncthreads();                                 // the chunk before has been read
        for (int t = (int)threadIdx.x; t < nm * KNOT_COLS; t += 256) {
            const int m = t / KNOT_COLS;
            const double kx = (double)(j0 + t % KNOT_COLS) * dk;
            double s, c;
            dsincos(kx * xy[2 * (m0 + m)], s, c);
            col_s[t] = s; col_c[t] = c;
        }
        for (int t = (int)threadIdx.x; t < nm * KNOT_ROWS; t += 256) {
            const int m = t / KNOT_ROWS, r = t % KNOT_ROWS;
            const int i = i0 + r;
            const double ky = (double)(i < n / 2 ? i : i - n) * dk;
            double s, c;
            dsincos(ky * xy[2 * (m0 + m) + 1], s, c);
            row_s[t] = s; row_c[t] = c;
        }
        __syncthreads();
        for (int m = 0; m < nm; ++m) {
            // exp(-i a) exp(-i b) = (ca cb - sa sb) - i (sa cb + ca sb)
            const double ca = col_c[m * KNOT_COLS + lane], sa = col_s[m * KNOT_COLS + lane];
#pragma unroll
            for (int r = 0; r < KNOT_PER_THREAD; ++r) {
                const double cb = row_c[m * KNOT_ROWS + r0 + r], sb = row_s[m * KNOT_ROWS + r0 + r];
                acc_re[r] = fma(-sa, sb, fma(ca, cb, acc_re[r]));
                acc_im[r] = fma(-ca, sb, fma(-sa, cb, acc_im[r]));
            }
        }
    }
    const int j = j0 + lane;
    if (j >= nh) return;
    const double dn = (double)N;
#pragma unroll
    for (int r = 0; r < KNOT_PER_THREAD; ++r) {
        const int i = i0 + r0 + r;
        if (i >= n) break;
        const double sr = acc_re[r] / dn, si = acc_im[r] / dn;
        const int64_t at = 2 * (o.k_offset + (int64_t)i * nh + j);
        const double re = kbuf[at], im = kbuf[at + 1];
        kbuf[at] = fma(re, sr, -(im * si));
        kbuf[at + 1] = fma(re, si, im * sr);
    }
}

extern "C" {

int ims_knot_positions(uint64_t seed, const ims_fft_object_t* objects_dev, int64_t n_objects, const int32_t* n_knots_dev,
                       const double* sigma_dev, const int64_t* knot_offset_dev, double* knot_xy_dev, void* stream)
{
    if (n_objects <= 0) return IMS_OK;
    if (!objects_dev || !n_knots_dev || !sigma_dev || !knot_offset_dev || !knot_xy_dev) return set_err(IMS_ERR_ARG, "NULL argument");
    if (n_objects > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "too many objects");
    hipLaunchKernelGGL(k_knot_positions, dim3((unsigned)n_objects), dim3(256), 0, (hipStream_t)stream, seed, objects_dev, n_knots_dev,
                       sigma_dev, knot_offset_dev, knot_xy_dev);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_fft_knots_factor(const ims_fft_params_t* params, const ims_fft_object_t* objects_dev, const int32_t* knot_rows_dev,
                         int64_t n_knot_rows, int32_t max_nfft, const int32_t* n_knots_dev, const int64_t* knot_offset_dev,
                         const double* knot_xy_dev, double* kbuf, void* stream)
{
    if (n_knot_rows <= 0) return IMS_OK;                             // no object with knots: nothing is launched
    if (!params || !objects_dev || !knot_rows_dev || !n_knots_dev || !knot_offset_dev || !knot_xy_dev || !kbuf)
        return set_err(IMS_ERR_ARG, "NULL argument");
    if (params->n_alias > 0) return set_err(IMS_ERR_UNSUPPORTED, "knots on the FFT branch need n_alias == 0 (the structure factor is no common factor of a folded spectrum)");
    if (max_nfft < 2 || (max_nfft & 1)) return set_err(IMS_ERR_ARG, "max_nfft must be even and >= 2");
    const unsigned gx = (unsigned)((max_nfft / 2 + 1 + KNOT_COLS - 1) / KNOT_COLS), gy = (unsigned)((max_nfft + KNOT_ROWS - 1) / KNOT_ROWS);
    if (gy > 65535u) return set_err(IMS_ERR_ARG, "max_nfft too large");
    for (int64_t first = 0; first < n_knot_rows; first += 65535) {
        const int64_t count = (n_knot_rows - first < 65535) ? n_knot_rows - first : 65535;
        hipLaunchKernelGGL(k_fft_knots_factor, dim3(gx, gy, (unsigned)count), dim3(256), 0, (hipStream_t)stream, *params, objects_dev,
                           knot_rows_dev + first, n_knots_dev, knot_offset_dev, knot_xy_dev, kbuf);
    }
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

}  // extern "C"
