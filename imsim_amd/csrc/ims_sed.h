// ims_sed.h -- per-object SED x extinction x throughput through the bandpass (ims_object_spectra): the flux of every object and
// the inverse CDF of its photon wavelengths, the table WavelengthSampler reads (ims_render_params_t.sed).  The device form of
// imsim_amd/sed.py:object_spectra, which restates InstCatalog.getSED / getObj (imsim/instcat.py:380-431, :563-573).
//
// One wavefront per object, SED_WAVES objects per workgroup, all arithmetic binary64.  A wavefront owns n_grid doubles of LDS:
//   1. density   lanes stride the band grid: the SED interpolated at grid / (1 + z) (bisection in the packed library, which
//                every object shares and which therefore stays in L2), times 10^(-0.4 Av (a + b / Rv)), times the throughput
//   2. sums      lane l owns the trapezoid segments [l m, (l + 1) m), m = ceil((n_grid - 1) / 64), and sums them in order
//   3. scan      the exclusive scan of the 64 lane sums, formed IN LANE ORDER: P[l + 1] = P[l] + S[l] (63 additions of a
//                wave-uniform value read with v_readlane).  A tree scan would be shorter but associates each prefix differently,
//                so P[l + 1] could fall an ulp below P[l] + S[l]: the stored CDF would then step down, or up, across a lane
//                boundary inside a plateau (zero density: an SED that ends inside the band), and the inversion's rule for
//                plateaus -- the bracket starts at the FIRST grid point that holds the value -- needs plateaus to be exact
//   4. CDF       the segments once more, the same additions, now stored as (P + running sum) / total over the densities
//   5. inversion lanes stride the n_pts abscissae u_j = j / (n_pts - 1): two bisections in LDS and one linear interpolation
// The CDF is non-decreasing by construction (fl(P + r) is monotone in r, and the last entry of lane l is fl(P[l] + S[l]) =
// P[l + 1]), and equal wherever the density is zero on both sides.
//
// A section of the one translation unit (imsim_hip.hip): the kernel in namespace ims, then its entry point ims_object_spectra.
#pragma once
#include "ims_math.h"

namespace ims {

constexpr int SED_WAVES = 4;                 // objects per workgroup
constexpr int SED_MAX_LDS = 64 * 1024;       // dynamic LDS a launch may ask for without an attribute of its own
constexpr double LN10 = 2.30258509299404568402;

struct SedArgs {
    const double* grid; const double* thr; const double* ext_a; const double* ext_b;
    const double* wave; const double* fphot; const int64_t* offset;
    const int32_t* sed_id; const double* redshift; const double* mw_av; const double* mw_rv;
    double* flux; double* tables;
    double band_hi;
    int64_t n_obj;
    int32_t n_grid, n_sed, n_pts, lds_stride;
};

// LDS traffic between the lanes of ONE wavefront: the hardware runs a wavefront's LDS instructions in order, so only the
// compiler has to be kept from moving them across this point
IMS_DEV void sed_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

IMS_DEV double sed_readlane(double v, int lane)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// np.interp(x, w[0 .. n), f[0 .. n), left = 0, right = 0)
IMS_DEV double sed_interp(const double* __restrict__ w, const double* __restrict__ f, int64_t n, double x)
{
    if (n <= 0 || !(x >= w[0]) || !(x <= w[n - 1])) return 0.0;      // (a NaN takes this way too: the search below needs w[0] <= x)
    if (x == w[n - 1]) return f[n - 1];
    int64_t lo = 0, hi = n - 1;              // w[lo] <= x < w[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (w[mid] <= x) lo = mid; else hi = mid;
    }
    const double slope = (f[lo + 1] - f[lo]) / (w[lo + 1] - w[lo]);
    return slope * (x - w[lo]) + f[lo];
}

__global__ __launch_bounds__(64 * SED_WAVES) void k_object_spectra(const SedArgs A)
{
    extern __shared__ double sed_lds[];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = (int)(threadIdx.x >> 6);
    const int64_t obj = (int64_t)blockIdx.x * SED_WAVES + wave;
    if (obj >= A.n_obj) return;               // wave-uniform; the kernel has no workgroup barrier
    double* __restrict__ cdf = sed_lds + (size_t)wave * A.lds_stride;
    double* __restrict__ row = A.tables + obj * (int64_t)A.n_pts;
    const int n_grid = A.n_grid, n_pts = A.n_pts;
    const int sid = A.sed_id[obj];
    if (sid < 0 || sid >= A.n_sed) {          // SED file not found: the caller's fallback
        if (lane == 0) A.flux[obj] = -1.0;
        for (int j = lane; j < n_pts; j += 64) row[j] = 0.0;
        return;
    }
    const int64_t s0 = A.offset[sid], sn = A.offset[sid + 1] - s0;
    const double* __restrict__ w = A.wave + s0;
    const double* __restrict__ f = A.fphot + s0;
    const double zp1 = 1.0 + A.redshift[obj];
    const double k_av = -0.4 * A.mw_av[obj], rv = A.mw_rv[obj];
    // 1. density on the grid
    for (int i = lane; i < n_grid; i += 64) {
        const double g = A.grid[i];
        const double spec = sed_interp(w, f, sn, g / zp1);
        const double ext = dexp((k_av * (A.ext_a[i] + A.ext_b[i] / rv)) * LN10);
        cdf[i] = spec * ext * A.thr[i];
    }
    sed_wave_sync();
    // 2. the lane's segments [k0, k1): segment k joins grid points k and k + 1
    const int nseg = n_grid - 1;
    const int m = (nseg + 63) / 64;
    const int k0 = min(lane * m, nseg), k1 = min(k0 + m, nseg);
    const double d_first = cdf[k0], d_last = cdf[k1];
    double S = 0.0;
    {
        double d_prev = d_first;
        for (int k = k0; k < k1; ++k) {
            const double d_next = cdf[k + 1];
            S = S + 0.5 * (d_next + d_prev) * (A.grid[k + 1] - A.grid[k]);
            d_prev = d_next;
        }
    }
    // 3. exclusive scan in lane order
    double P = 0.0, run = 0.0;
#pragma unroll
    for (int l = 0; l < 63; ++l) {
        run = run + sed_readlane(S, l);
        if (lane == l + 1) P = run;
    }
    const double total = run + sed_readlane(S, 63);
    if (lane == 0) A.flux[obj] = total;
    const double lo = A.grid[0];
    if (!(total > 0.0)) {                     // nothing through the band: np.linspace(lo, hi, n_pts)
        const double step = (A.band_hi - lo) / (double)(n_pts - 1);
        for (int j = lane; j < n_pts; j += 64) row[j] = (j == n_pts - 1) ? A.band_hi : (double)j * step + lo;
        return;
    }
    sed_wave_sync();                          // every lane holds d_first / d_last: the densities may be overwritten
    // 4. the normalised CDF in place of the densities.  Lane l writes (k0, k1]; entry k1 is lane l + 1's d_first
    if (lane == 0) cdf[0] = 0.0;
    {
        double d_prev = d_first, r = 0.0;
        for (int k = k0; k < k1; ++k) {
            const double d_next = (k + 1 == k1) ? d_last : cdf[k + 1];
            r = r + 0.5 * (d_next + d_prev) * (A.grid[k + 1] - A.grid[k]);
            cdf[k + 1] = (P + r) / total;
            d_prev = d_next;
        }
    }
    sed_wave_sync();
    // 5. np.interp(u, c[keep], grid[keep]): a knot is kept when it is the first or exceeds its predecessor
    const double ustep = 1.0 / (double)(n_pts - 1);
    for (int j = lane; j < n_pts; j += 64) {
        const double u = (j == n_pts - 1) ? 1.0 : (double)j * ustep;
        int a = 0, b = n_grid;                // first index with cdf > u (cdf[0] = 0 <= u): n_grid when u reaches the maximum
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (cdf[mid] <= u) a = mid + 1; else b = mid;
        }
        const int i1 = a;
        const double v0 = cdf[i1 - 1];
        a = 0; b = i1 - 1;                    // first index that holds v0: the kept knot of its plateau
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (cdf[mid] < v0) a = mid + 1; else b = mid;
        }
        const int i0 = a;
        const double g0 = A.grid[i0];
        double val = g0;                      // u at the maximum: the first grid point that reaches it
        if (i1 < n_grid) {
            const double slope = (A.grid[i1] - g0) / (cdf[i1] - v0);
            val = slope * (u - v0) + g0;
        }
        row[j] = val;
    }
}

}  // namespace ims

extern "C" {

int ims_object_spectra(const double* grid, const double* thr, const double* ext_a, const double* ext_b, int32_t n_grid, double band_hi,
                       const double* sed_wave, const double* sed_fphotons, const int64_t* sed_offset, int32_t n_sed,
                       const int32_t* sed_id, const double* redshift, const double* mw_av, const double* mw_rv, int64_t n_obj,
                       int32_t n_pts, double* flux, double* tables, int64_t row_offset, void* stream)
{
    if (n_obj < 0 || row_offset < 0) return set_err(IMS_ERR_ARG, "object spectra: negative object count or row offset");
    if (n_obj == 0) return IMS_OK;
    if (!grid || !thr || !ext_a || !ext_b || !sed_offset || !sed_id || !redshift || !mw_av || !mw_rv || !flux || !tables)
        return set_err(IMS_ERR_ARG, "object spectra: an array is NULL");
    if (n_sed < 0 || (n_sed > 0 && (!sed_wave || !sed_fphotons))) return set_err(IMS_ERR_ARG, "object spectra: the SED library is NULL");
    if (n_grid < 2 || n_pts < 2) return set_err(IMS_ERR_ARG, "object spectra: the band grid and the tables need two points at least");
    if ((int64_t)n_grid * SED_WAVES * (int64_t)sizeof(double) > SED_MAX_LDS) {
        snprintf(g_err, sizeof(g_err), "object spectra: a band grid of %d points does not fit the %d doubles of LDS a wavefront has "
                 "(a coarser step or a narrower band)", (int)n_grid, (int)(SED_MAX_LDS / (SED_WAVES * sizeof(double))));
        return IMS_ERR_UNSUPPORTED;
    }
    const int64_t blocks = (n_obj + SED_WAVES - 1) / SED_WAVES;
    if (blocks > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "object spectra: too many objects for one launch");
    SedArgs A;
    A.grid = grid; A.thr = thr; A.ext_a = ext_a; A.ext_b = ext_b;
    A.wave = sed_wave; A.fphot = sed_fphotons; A.offset = sed_offset;
    A.sed_id = sed_id; A.redshift = redshift; A.mw_av = mw_av; A.mw_rv = mw_rv;
    A.flux = flux; A.tables = tables + row_offset * (int64_t)n_pts;
    A.band_hi = band_hi; A.n_obj = n_obj;
    A.n_grid = n_grid; A.n_sed = n_sed; A.n_pts = n_pts; A.lds_stride = n_grid;
    hipLaunchKernelGGL(k_object_spectra, dim3((unsigned)blocks), dim3(64 * SED_WAVES), (size_t)n_grid * SED_WAVES * sizeof(double),
                       (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

}  // extern "C"
