// ims_stamp_fft.h -- section of the one translation unit (imsim_hip.hip): FITS-stamp objects (IMS_PROF_IMAGE) on the FFT branch.
//
// A stamp object is galsim.InterpolatedImage: a finite lattice of interpolant kernels, one per pixel, weighted by the pixel.  Its
// continuous spectrum is
//     F(k) = [ sum_m w_m exp(-i k . d_m) ] Qhat(q_u p / 2 pi) Qhat(q_v p / 2 pi),      q = J'^T k,
// w_m the non-negative pixels normalised to sum 1 (what image_sample draws from), d_m = J' (p (a + 1/2 - w / 2), p (b + 1/2 - h / 2)) the
// pixel centres of image_sample along the CCD's pixel axes [arcsec], p the stamp's pixel scale (ims_fft_object_t.prof_scale), J' the
// FFT row's affine and Qhat the transform of the interpolant: the quintic's closed form, or sinc for the nearest interpolant (a photon
// lands uniformly inside its pixel).  ims_fft_kspace_fill fills such an object as a point (prof_ktable IMS_PROF_POINT); the pass here
// multiplies its half spectrum by F before the inverse transform.  Base band only (ims_fft_params_t.n_alias == 0): F at k + a ks is not
// a common factor of a folded sum.
//
// Kernel: k_fft_image_factor.  Entry point: ims_fft_image_factor.
#pragma once

// sin(pi u) / (pi u) and cos(pi u) for u >= 0.  pi u = 2 pi (u / 2): the halving and the fraction of a turn are exact, so the sine is
// good relative to its distance from the zero at every integer u (sincos2pi reduces the quadrant exactly).
IMS_DEV void sinc_cos_pi(double u, double& sn, double& cs)
{
    if (u == 0.0) { sn = 1.0; cs = 1.0; return; }
    double t = 0.5 * u;
    t = t - floor(t);
    double s;
    sincos2pi(t, s, cs);
    sn = s / (0.5 * TWO_PI * u);
}

// Transform of GalSim's Quintic interpolant (Bernstein & Gruen 2014) at u cycles per stamp pixel, from the piecewise quintic
// integrated by parts:  Qhat(u) = s^5 (s (55 - 19 x^2) + 2 cos(x) (x^2 - 27)),  x = pi u, s = sin(x) / x.  Qhat(0) = 55 - 54 = 1, and
// Qhat(j) = 0 at every other integer (s = 0 there: the kernel reproduces constants).  Even in u.
// At u -> 0 the bracket is 55 s - 54 c + O(x^2): two terms of ~55 rounded apart, an absolute error of some 1e-14 on a value of 1.
IMS_DEV double quintic_hat(double u)
{
    double s, c;
    sinc_cos_pi(fabs(u), s, c);
    const double x = 0.5 * TWO_PI * u, x2 = x * x, s2 = s * s;
    return s * s2 * s2 * fma(s, fma(-19.0, x2, 55.0), 2.0 * c * (x2 - 27.0));
}
IMS_DEV double nearest_hat(double u)
{
    double s, c;
    sinc_cos_pi(fabs(u), s, c);
    return s;
}

// The pass.  Ownership and LDS layout are k_fft_knots_factor's (ims_knots.h): a workgroup owns STAMP_ROWS x STAMP_COLS points of ONE
// object's half spectrum (blockIdx.z: the object's place in the list of rows with a stamp; tiles beyond the object's own grid leave at
// once).  The stamp's positive pixels come in chunks of STAMP_CHUNK.  Per chunk the first STAMP_CHUNK threads stage d_m and w_m in LDS
// (J' . (a, b) once per pixel, not once per column); then the workgroup forms w_m exp(-i kx_j dx_m) for the tile's columns -- the
// weight folded in as the phase is stored -- and exp(-i ky_i dy_m) for its rows, ONCE each (one dsincos per (pixel, column) and per
// (pixel, row)); then every thread accumulates its column against STAMP_ROWS / 4 rows with four v_fma_f64 per (pixel, cell).
// LDS: cosines and sines apart, [pixel][column]: the 64 lanes of a wavefront read 64 consecutive doubles (ds_read_b64: two halves of
// 32 lanes x 8 B = one 256-B bank row each, no conflict); the row phases are read at a wave-uniform address (a broadcast).
// 48 KB + 768 B per workgroup: three workgroups on a CU's 160 KB, as the knots pass.
// The sum of a point runs over the pixels ascending (row-major over the stamp) with one association, whatever the tile or the chunk:
// the result does not depend on the launch geometry.
constexpr int STAMP_ROWS = 32, STAMP_COLS = 64, STAMP_CHUNK = 32, STAMP_PER_THREAD = STAMP_ROWS / 4;
__global__ __launch_bounds__(256) void k_fft_image_factor(const ims_fft_params_t P, const ims_fft_object_t* __restrict__ objs,
                                                          const int32_t* __restrict__ image_rows, const int32_t* __restrict__ row_image,
                                                          int32_t n_images, const int32_t* __restrict__ image_size,
                                                          const int64_t* __restrict__ image_offset, const int32_t* __restrict__ pixel_ab,
                                                          const double* __restrict__ pixel_w, int32_t interpolant, double* __restrict__ kbuf)
{
    __shared__ double col_c[STAMP_CHUNK * STAMP_COLS], col_s[STAMP_CHUNK * STAMP_COLS];
    __shared__ double row_c[STAMP_CHUNK * STAMP_ROWS], row_s[STAMP_CHUNK * STAMP_ROWS];
    __shared__ double pix_x[STAMP_CHUNK], pix_y[STAMP_CHUNK], pix_f[STAMP_CHUNK];
    const int32_t oi = image_rows[blockIdx.z];
    const ims_fft_object_t& o = objs[oi];
    const int n = o.nfft, nh = n / 2 + 1;
    const int j0 = (int)blockIdx.x * STAMP_COLS, i0 = (int)blockIdx.y * STAMP_ROWS;
    const int32_t img = row_image[oi];
    if (j0 >= nh || i0 >= n || img < 0 || img >= n_images) return;   // (uniform over the workgroup)
    const int64_t first = image_offset[img];
    const int32_t N = (int32_t)(image_offset[img + 1] - first);
    const double half_w = 0.5 * (double)image_size[2 * img], half_h = 0.5 * (double)image_size[2 * img + 1];
    const double p = o.prof_scale;
    const double dk = TWO_PI / ((double)n * P.pixel_scale);
    const int lane = (int)(threadIdx.x & 63u);
    const int r0 = (int)(threadIdx.x >> 6) * STAMP_PER_THREAD;       // first of this wavefront's rows inside the tile
    double acc_re[STAMP_PER_THREAD], acc_im[STAMP_PER_THREAD];
#pragma unroll
    for (int r = 0; r < STAMP_PER_THREAD; ++r) { acc_re[r] = 0.0; acc_im[r] = 0.0; }
    for (int32_t m0 = 0; m0 < N; m0 += STAMP_CHUNK) {
        const int nm = (N - m0 < STAMP_CHUNK) ? (int)(N - m0) : STAMP_CHUNK;
        if (m0 > 0) __syncthreads();                                 // the chunk before has been read
        if ((int)threadIdx.x < nm) {
            // the pixel's centre as image_sample has it (in stamp pixels from the stamp's centre), then p, then J'
            const int64_t m = first + m0 + (int64_t)threadIdx.x;
            const double gx = p * (((double)pixel_ab[2 * m] + 0.5) - half_w), gy = p * (((double)pixel_ab[2 * m + 1] + 0.5) - half_h);
            pix_x[threadIdx.x] = o.jac[0] * gx + o.jac[1] * gy;
            pix_y[threadIdx.x] = o.jac[2] * gx + o.jac[3] * gy;
            pix_f[threadIdx.x] = pixel_w[m];
        }
        __syncthreads();
        for (int t = (int)threadIdx.x; t < nm * STAMP_COLS; t += 256) {
            const int m = t / STAMP_COLS;
            const double kx = (double)(j0 + t % STAMP_COLS) * dk;
            double s, c;
            dsincos(kx * pix_x[m], s, c);
            const double f = pix_f[m];
            col_s[t] = f * s; col_c[t] = f * c;
        }
        for (int t = (int)threadIdx.x; t < nm * STAMP_ROWS; t += 256) {
            const int m = t / STAMP_ROWS, r = t % STAMP_ROWS;
            const int i = i0 + r;
            const double ky = (double)(i < n / 2 ? i : i - n) * dk;
            double s, c;
            dsincos(ky * pix_y[m], s, c);
            row_s[t] = s; row_c[t] = c;
        }
        __syncthreads();
        for (int m = 0; m < nm; ++m) {
            // w exp(-i a) exp(-i b) = w (ca cb - sa sb) - i w (sa cb + ca sb)
            const double ca = col_c[m * STAMP_COLS + lane], sa = col_s[m * STAMP_COLS + lane];
#pragma unroll
            for (int r = 0; r < STAMP_PER_THREAD; ++r) {
                const double cb = row_c[m * STAMP_ROWS + r0 + r], sb = row_s[m * STAMP_ROWS + r0 + r];
                acc_re[r] = fma(-sa, sb, fma(ca, cb, acc_re[r]));
                acc_im[r] = fma(-ca, sb, fma(-sa, cb, acc_im[r]));
            }
        }
    }
    const int j = j0 + lane;
    if (j >= nh) return;
    const double kx = (double)j * dk;
    const double cyc = p * INV_TWO_PI;                               // q p / 2 pi: cycles per stamp pixel
#pragma unroll
    for (int r = 0; r < STAMP_PER_THREAD; ++r) {
        const int i = i0 + r0 + r;
        if (i >= n) break;
        const double ky = (double)(i < n / 2 ? i : i - n) * dk;
        const double u = (o.jac[0] * kx + o.jac[2] * ky) * cyc, v = (o.jac[1] * kx + o.jac[3] * ky) * cyc;
        const double q = (interpolant != 0) ? quintic_hat(u) * quintic_hat(v) : nearest_hat(u) * nearest_hat(v);
        const double sr = acc_re[r] * q, si = acc_im[r] * q;
        const int64_t at = 2 * (o.k_offset + (int64_t)i * nh + j);
        const double re = kbuf[at], im = kbuf[at + 1];
        kbuf[at] = fma(re, sr, -(im * si));
        kbuf[at + 1] = fma(re, si, im * sr);
    }
}

extern "C" {

int ims_fft_image_factor(const ims_fft_params_t* params, const ims_fft_object_t* objects_dev, const int32_t* image_rows_dev,
                         int64_t n_image_rows, int32_t max_nfft, const int32_t* row_image_dev, int32_t n_images,
                         const int32_t* image_size_dev, const int64_t* image_offset_dev, const int32_t* pixel_ab_dev,
                         const double* pixel_w_dev, int32_t interpolant, double* kbuf, void* stream)
{
    if (n_image_rows <= 0) return IMS_OK;                            // no object with a stamp: nothing is launched
    if (!params || !objects_dev || !image_rows_dev || !row_image_dev || !image_size_dev || !image_offset_dev || !pixel_ab_dev ||
        !pixel_w_dev || !kbuf)
        return set_err(IMS_ERR_ARG, "NULL argument");
    if (params->n_alias > 0) return set_err(IMS_ERR_UNSUPPORTED, "FITS stamps on the FFT branch need n_alias == 0 (the stamp's spectrum is no common factor of a folded spectrum)");
    if (max_nfft < 2 || (max_nfft & 1)) return set_err(IMS_ERR_ARG, "max_nfft must be even and >= 2");
    if (n_images <= 0) return set_err(IMS_ERR_ARG, "n_images must be positive");
    if (interpolant != 0 && interpolant != 1) return set_err(IMS_ERR_ARG, "interpolant: 0 (nearest) or 1 (quintic)");
    const unsigned gx = (unsigned)((max_nfft / 2 + 1 + STAMP_COLS - 1) / STAMP_COLS), gy = (unsigned)((max_nfft + STAMP_ROWS - 1) / STAMP_ROWS);
    if (gy > 65535u) return set_err(IMS_ERR_ARG, "max_nfft too large");
    for (int64_t first = 0; first < n_image_rows; first += 65535) {
        const int64_t count = (n_image_rows - first < 65535) ? n_image_rows - first : 65535;
        hipLaunchKernelGGL(k_fft_image_factor, dim3(gx, gy, (unsigned)count), dim3(256), 0, (hipStream_t)stream, *params, objects_dev,
                           image_rows_dev + first, row_image_dev, n_images, image_size_dev, image_offset_dev, pixel_ab_dev, pixel_w_dev,
                           interpolant, kbuf);
    }
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

}  // extern "C"
