// ims_test.h -- section of the one translation unit (imsim_hip.hip): device probes of the parity tests.
//
// Kernels: k_test_math, k_test_optical_screen.
// Entry points: ims_test_math, ims_test_optical_screen.
#pragma once

// device math probe for the parity tests (which: 0 log,1 exp,2 sincos2pi,3 atan,4 sincos,5 tanh,6 gauss,7 dsqrt_n,8 ddiv of pairs,9 dsqrt0,
// 10 sincos2pi of a word,11 log of a word,12 gauss_word_cos of pairs,13 dlgamma,14 atan2 of pairs,15 pow of pairs,16 Philox block of quads)
__global__ void k_test_math(int which, const double* __restrict__ in, double* __restrict__ out, int64_t n,
                            uint64_t seed, int64_t obj, uint32_t slot)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s, c;
    switch (which) {
    case 0: out[i] = dlog(in[i]); break;
    case 1: out[i] = dexp(in[i]); break;
    case 2: sincos2pi(in[i], s, c); out[2 * i] = s; out[2 * i + 1] = c; break;
    case 3: out[i] = datan(in[i]); break;
    case 4: dsincos(in[i], s, c); out[2 * i] = s; out[2 * i + 1] = c; break;
    case 5: out[i] = dtanh_pos(in[i]); break;
    case 7: out[i] = dsqrt_n(in[i]); break;
    case 8: out[i] = ddiv(in[2 * i], in[2 * i + 1]); break;
    case 9: out[i] = dsqrt0(in[i]); break;
    case 6: { Rng r; rng_reset(r); rng_block(r, seed, obj, i, slot); gauss_words(r.w[0], r.w[1], s, c);
              out[2 * i] = s; out[2 * i + 1] = c; break; }
    // the deviate functions of spec v6; the words come as integer-valued doubles
    case 10: sincos2pi_w((uint32_t)in[i], s, c); out[2 * i] = s; out[2 * i + 1] = c; break;
    case 11: out[i] = dlog_w((uint32_t)in[i]); break;
    case 12: out[i] = gauss_word_cos((uint32_t)in[2 * i], (uint32_t)in[2 * i + 1]); break;
    // log Gamma of the Poisson deviate's acceptance test (x > 0)
    case 13: out[i] = dlgamma(in[i]); break;
    case 14: out[i] = datan2(in[2 * i], in[2 * i + 1]); break;       // pairs (y, x)
    case 15: out[i] = dpow(in[2 * i], in[2 * i + 1]); break;         // pairs (x, y)
    // the raw Philox block of four integer-valued doubles (photon low word, photon high word, slot, object low word); the seed and
    // the object's high word come through `seed` and `obj` (its low word is replaced by the point's): four words out
    case 16: {
        const uint64_t photon = (uint64_t)(uint32_t)in[4 * i] | ((uint64_t)(uint32_t)in[4 * i + 1] << 32);
        const uint64_t id = ((uint64_t)obj & 0xFFFFFFFF00000000ull) | (uint64_t)(uint32_t)in[4 * i + 3];
        // an empty cache is marked by slot 0xFFFFFFFF (rng_reset), which no kernel uses but the second Random123 vector has:
        // mark it with another slot than the one asked for
        const uint32_t slot_i = (uint32_t)in[4 * i + 2];
        Rng r; rng_reset(r); r.slot = ~slot_i; rng_block(r, seed, (int64_t)id, (int64_t)photon, slot_i);
        for (int j = 0; j < 4; ++j) out[4 * i + j] = (double)r.w[j];
        break; }
    }
}

// the optical phase screen's device functions (ims_optical.h) on n independent points, one thread each: the same functions, in
// the same order, as optical_setup and apply_psf_optical run them (there a workgroup shares the per-object part through LDS)
__global__ __launch_bounds__(256) void k_test_optical_screen(const ims_optical_screen_t* __restrict__ screen,
                                                             const double* __restrict__ thx, const double* __restrict__ thy,
                                                             const double* __restrict__ u, const double* __restrict__ v, int64_t n,
                                                             double* __restrict__ coef, double* __restrict__ dwdu,
                                                             double* __restrict__ dwdv)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    OptScreenPtr S = (OptScreenPtr)screen;
    const double tx = optical_theta(S, thx[i]), ty = optical_theta(S, thy[i]);
    double a[IMS_OPT_NZ], gxc[21], gyc[21];
    for (int j = 0; j < IMS_OPT_NZ; ++j) { a[j] = optical_coeff(S, j, tx, ty); coef[i * IMS_OPT_NZ + j] = a[j]; }
    for (int t = 0; t < IMS_OPT_NPUPIL; ++t) optical_gradient_coeff(t, optical_pupil_coeff(S, (const double*)a, t), (double*)gxc, (double*)gyc);
    double gx, gy;
    optical_gradient((const double*)gxc, (const double*)gyc, S->inv_r, S->grad_scale, u[i], v[i], gx, gy);
    dwdu[i] = gx; dwdv[i] = gy;
}

extern "C" {

int ims_test_math(int which, const double* in_dev, double* out_dev, int64_t n, uint64_t seed, int64_t obj,
                  uint32_t slot, void* stream)
{
    if (n <= 0) return IMS_OK;
    hipLaunchKernelGGL(k_test_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       which, in_dev, out_dev, n, seed, obj, slot);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_test_optical_screen(const ims_optical_screen_t* screen_dev, const double* thx, const double* thy, const double* u,
                            const double* v, int64_t n, double* coef, double* dwdu, double* dwdv, void* stream)
{
    if (n <= 0) return IMS_OK;
    if (!screen_dev || !thx || !thy || !u || !v || !coef || !dwdu || !dwdv) return set_err(IMS_ERR_ARG, "optical screen probe: NULL argument");
    hipLaunchKernelGGL(k_test_optical_screen, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       screen_dev, thx, thy, u, v, n, coef, dwdu, dwdv);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

}  // extern "C"
