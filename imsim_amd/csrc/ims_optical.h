// The optical phase screen of AtmosphericPSF(doOpt=True) (IMS_PSF_OPTICAL_SCREEN; include/imsim_hip.h, ims_optical_screen_t):
// imSim's OptWF (imsim/atmPSF.py:37-76) restated.  Included by ims_photon.h between apply_psf and run_psf.
//
// Per object (wave-uniform): the 19 annular-Zernike coefficients at the object's field angle and from them the 2 x 21 monomial
// coefficients of the two gradient polynomials -- formed ONCE per workgroup, the 256 threads together, into 512 bytes of LDS
// (optical_setup; ~290 multiply-adds for the coefficients, ~530 for the pupil monomials, spread over 19 and 28 lanes).  Per photon:
// two bivariate Horner evaluations of degree 5 (40 fma) on coefficients broadcast from LDS.  Kernels that are not compiled for
// the component (run_psf<0..2>) never reference anything in this file and allocate none of its LDS.
#pragma once

constexpr int OPT_LDS_A = 0;                                   // a_4 .. a_22
constexpr int OPT_LDS_GX = IMS_OPT_NZ;                         // 21 coefficients of dP/dx, rows IMS_OPT_ROW(5, q)
constexpr int OPT_LDS_GY = OPT_LDS_GX + 21;
constexpr int OPT_LDS_INV_R = OPT_LDS_GY + 21;
constexpr int OPT_LDS_GRAD_SCALE = OPT_LDS_INV_R + 1;
constexpr int OPT_LDS_N = 64;
constexpr double OPT_DEG_PER_RAD = 57.29577951308232;

typedef const IMS_G ims_optical_screen_t* OptScreenPtr;
IMS_DEV OptScreenPtr optical_of(const ims_atmosphere_t* A)
{
    return (OptScreenPtr)&reinterpret_cast<const ims_atmosphere_optical_t*>(A)->opt;
}

// one allocation per kernel that calls it (the setup and the per-photon kick of a kernel see the same block)
IMS_DEV double* optical_lds()
{
    __shared__ double block[OPT_LDS_N];
    return block;
}

// sum_{p + q <= DEG} c[IMS_OPT_ROW(DEG, q) + p] x^p y^q: every row by Horner in x from its highest power, then the rows by
// Horner in y from the highest; FMA: each step one fma(acc, x, c), else a rounded product and a rounded sum
template <int DEG, bool FMA, typename PTR>
IMS_DEV double optical_poly(PTR c, double x, double y)
{
    double acc = 0.0;
#pragma unroll
    for (int q = DEG; q >= 0; --q) {
        double s = c[IMS_OPT_ROW(DEG, q) + (DEG - q)];
#pragma unroll
        for (int p = DEG - q - 1; p >= 0; --p) s = FMA ? fma(s, x, c[IMS_OPT_ROW(DEG, q) + p]) : s * x + c[IMS_OPT_ROW(DEG, q) + p];
        if (q == DEG) acc = s;
        else acc = FMA ? fma(acc, y, s) : acc * y + s;
    }
    return acc;
}

// remapped field angle [deg] of an object
IMS_DEV double optical_theta(OptScreenPtr S, double atm_tan) { return (atm_tan * OPT_DEG_PER_RAD) * S->remap; }

// a_j at the remapped field angle (thx, thy) [deg]
IMS_DEV double optical_coeff(OptScreenPtr S, int j, double thx, double thy)
{
    return optical_poly<4, false>((const IMS_G double*)S->field[j], thx, thy);
}

// w_t = sum_j a_j pupil[j][t], j in order
template <typename APTR>
IMS_DEV double optical_pupil_coeff(OptScreenPtr S, APTR a, int t)
{
    double w = a[0] * S->pupil[0][t];
    for (int j = 1; j < IMS_OPT_NZ; ++j) w = w + a[j] * S->pupil[j][t];
    return w;
}

// monomial t of the degree-6 layout is x^p y^q: its contributions (double)p * w to dP/dx at x^(p-1) y^q and (double)q * w to
// dP/dy at x^p y^(q-1); every entry of gx / gy is written by exactly one t
template <typename GPTR>
IMS_DEV void optical_gradient_coeff(int t, double w, GPTR gx, GPTR gy)
{
    int q = 0;
    while (q < 6 && IMS_OPT_ROW(6, q + 1) <= t) ++q;
    const int p = t - IMS_OPT_ROW(6, q);
    if (p >= 1) gx[IMS_OPT_ROW(5, q) + (p - 1)] = (double)p * w;
    if (q >= 1) gy[IMS_OPT_ROW(5, q - 1) + p] = (double)q * w;
}

// wavefront gradient [nm/m] at the pupil position (pu, pv) [m]
template <typename GPTR>
IMS_DEV void optical_gradient(GPTR gxc, GPTR gyc, double inv_r, double grad_scale, double pu, double pv, double& gx, double& gy)
{
    const double x = pu * inv_r, y = pv * inv_r;
    gx = grad_scale * optical_poly<5, true>(gxc, x, y);
    gy = grad_scale * optical_poly<5, true>(gyc, x, y);
}

// Called by ALL threads of a workgroup whose photons belong to object o, before any of them leaves the kernel.
IMS_DEV void optical_setup(const ims_render_params_t& P, const ims_object_t& o)
{
    double* L = optical_lds();
    OptScreenPtr S = optical_of(P.atm);
    const int t = (int)threadIdx.x;
    if (t < IMS_OPT_NZ) {
        const double thx = optical_theta(S, o.atm_tan_x), thy = optical_theta(S, o.atm_tan_y);
        L[OPT_LDS_A + t] = optical_coeff(S, t, thx, thy);
    } else if (t == 32) {
        L[OPT_LDS_INV_R] = S->inv_r;
        L[OPT_LDS_GRAD_SCALE] = S->grad_scale;
    }
    __syncthreads();
    if (t < IMS_OPT_NPUPIL) optical_gradient_coeff(t, optical_pupil_coeff(S, L + OPT_LDS_A, t), L + OPT_LDS_GX, L + OPT_LDS_GY);
    __syncthreads();
}

// The component's kick.  have_pupil: an IMS_PSF_SCREENS component earlier in the list has set ph.pu / ph.pv.
IMS_DEV void apply_psf_optical(const ims_render_params_t& P, const ims_object_t& o, int comp, int64_t k, bool have_pupil, Rng& rng,
                               Photon& ph)
{
    const ims_psf_component_t& c = P.psf[comp];
    const double* L = optical_lds();
    if (!have_pupil) {
        const ims_atmosphere_t& A = *P.atm;
        rng_block(rng, P.seed, o.obj_id, k, SLOT_PSF + (uint32_t)(IMS_MAX_PSF >> 1));
        const double r = dsqrt0(A.aper_ri2 + w01(rng.w[0]) * A.aper_dr2);
        double s, cc;
        sincos2pi_w(rng.w[1], s, cc);
        ph.pu = r * cc; ph.pv = r * s;
    }
    double gx, gy;
    optical_gradient(L + OPT_LDS_GX, L + OPT_LDS_GY, L[OPT_LDS_INV_R], L[OPT_LDS_GRAD_SCALE], ph.pu, ph.pv, gx, gy);
    const double ku = c.p0 * gx, kv = c.p0 * gy;
    ph.x = ph.x + (o.winv[0] * ku + o.winv[1] * kv);
    ph.y = ph.y + (o.winv[2] * ku + o.winv[3] * kv);
}
