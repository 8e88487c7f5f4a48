// ims_image.h -- section of the one translation unit (imsim_hip.hip): LSST_Flat and the image utilities.
//
// Kernels: k_pixel_areas (Silicon::fillWithPixelAreas of one slot), k_flat_add (a Poisson flat level, optionally times a base image
// and the pixel areas), k_image_add, k_image_to_float, k_paint_cosmic_rays (one workgroup per hit of a layer).
// Entry points: ims_sensor_pixel_areas, ims_flat_add, ims_image_add, ims_paint_cosmic_rays, ims_image_to_float.
#pragma once

// ---------------- LSST_Flat ----------------
constexpr long long FLAT_ID_BASE = 0x7F00000000ll;      // object id space of the flat builder's Poisson streams

// Silicon::fillWithPixelAreas: shoelace area of the (distorted) polygon of every pixel of one slot
__global__ __launch_bounds__(256) void k_pixel_areas(const ims_sensor_t* __restrict__ sp, int slot, double* __restrict__ area,
                                                     long long* __restrict__ sum_q32)
{
    const ims_sensor_t& s = *sp;
    const ims_bf_slot_t bs = s.bf_slots[slot];
    const SlotView sl = { bs.xmin, bs.ymin, bs.nx, bs.ny, bs.offset };
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)sl.nx * sl.ny) return;
    const int i = (int)(p % sl.nx), j = (int)(p / sl.nx);
    const int nv = 4 * s.num_vertices + 4;
    double x0, y0, xp, yp, a2 = 0.0;
    polygon_vertex(s, sl, i, j, 0, 1.0, x0, y0);
    xp = x0; yp = y0;
    for (int k = 1; k <= nv; ++k) {
        double xk = x0, yk = y0;
        if (k < nv) polygon_vertex(s, sl, i, j, k, 1.0, xk, yk);
        a2 = a2 + (xp * yk - xk * yp);
        xp = xk; yp = yk;
    }
    const double a = 0.5 * a2;
    area[p] = a;
    atomicAdd((unsigned long long*)sum_q32, (unsigned long long)(long long)floor(a * 0x1.0p32 + 0.5));
}

__global__ __launch_bounds__(256) void k_flat_add(const double* __restrict__ area, const double* __restrict__ base, double level,
                                                  double inv_mean_area, uint64_t seed, int64_t iteration, int nx, int ny,
                                                  double* __restrict__ image, double* __restrict__ delta)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)nx * ny) return;
    double mean = level;
    if (base != nullptr) mean = mean * base[p];
    if (area != nullptr) mean = mean * (area[p] * inv_mean_area);
    const double v = poisson(mean, seed, FLAT_ID_BASE + iteration, p);
    image[p] = image[p] + v;
    if (delta != nullptr) {
        const int i = (int)(p % nx), j = (int)(p / nx);
        delta[(int64_t)j * (nx + 1) + i] = delta[(int64_t)j * (nx + 1) + i] + v;
    }
}

__global__ __launch_bounds__(256) void k_image_add(double* __restrict__ dst, const double* __restrict__ src, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] += src[i];
}

__global__ __launch_bounds__(256) void k_image_to_float(const double* __restrict__ src, float* __restrict__ dst, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = (float)src[i];
}

// One workgroup per hit of a layer, a lane per span pixel.  The hits of a layer cover disjoint pixels (the caller's layering),
// so the plain read-add-write below has no races, and each pixel sees its adds in layer order.  A footprint has some tens of
// pixels: one wave per hit, the span of a pixel by binary search over the footprint's pixel prefix.
__global__ __launch_bounds__(64) void k_paint_cosmic_rays(double* __restrict__ image, int32_t nx, int32_t ny,
                                                          const ims_cr_span_t* __restrict__ spans, int64_t n_spans,
                                                          const double* __restrict__ values, int64_t n_values,
                                                          const ims_cr_hit_t* __restrict__ hits)
{
    const ims_cr_hit_t h = hits[blockIdx.x];
    if (h.n_spans < 1 || h.first_span < 0 || (int64_t)h.first_span + h.n_spans > n_spans) return;
    const int32_t base = spans[h.first_span].first_pixel;
    for (int32_t k = threadIdx.x; k < h.n_pixels; k += blockDim.x) {
        int32_t lo = h.first_span, hi = h.first_span + h.n_spans - 1;        // last span whose first pixel is <= k
        while (lo < hi) {
            const int32_t mid = lo + (hi - lo + 1) / 2;
            if (spans[mid].first_pixel - base <= k) lo = mid;
            else hi = mid - 1;
        }
        const ims_cr_span_t s = spans[lo];
        const int32_t dx = k - (s.first_pixel - base);
        if (dx < 0 || dx >= s.n || s.value_offset < 0 || s.value_offset + dx >= n_values) continue;
        const int64_t row = (int64_t)h.y0 + s.row, col = (int64_t)h.x0 + s.col + dx;
        if (row < 0 || row >= ny || col < 0 || col >= nx) continue;
        image[row * nx + col] += values[s.value_offset + dx];
    }
}

extern "C" {

int ims_sensor_pixel_areas(const ims_sensor_t* sensor_dev, const ims_sensor_t* sensor_host, int32_t slot,
                           double* area_dev, long long* sum_q32_dev, void* stream)
{
    if (!sensor_dev || !area_dev || !sum_q32_dev) return set_err(IMS_ERR_ARG, "NULL argument");
    if (!sensor_host || !sensor_host->bf_slots) return set_err(IMS_ERR_ARG, "sensor_host/bf_slots is NULL (host copy of the slot table required)");
    if (slot < 0 || slot >= sensor_host->n_bf_slots) return set_err(IMS_ERR_ARG, "slot out of range");
    const ims_bf_slot_t& b = sensor_host->bf_slots[slot];
    const int64_t n = (int64_t)b.nx * b.ny;
    if (n <= 0) return IMS_OK;
    hipLaunchKernelGGL(k_pixel_areas, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sensor_dev, slot,
                       area_dev, sum_q32_dev);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_flat_add(const double* area_dev, const double* base_dev, double level, double inv_mean_area, uint64_t seed,
                 int64_t iteration, int32_t nx, int32_t ny, double* image_dev, double* delta_dev, void* stream)
{
    if (!image_dev) return set_err(IMS_ERR_ARG, "image is NULL");
    if (nx <= 0 || ny <= 0) return IMS_OK;
    const int64_t n = (int64_t)nx * ny;
    hipLaunchKernelGGL(k_flat_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, area_dev, base_dev,
                       level, inv_mean_area, seed, iteration, nx, ny, image_dev, delta_dev);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_image_add(double* dst, const double* src, int64_t n, void* stream)
{
    if (!dst || !src) return set_err(IMS_ERR_ARG, "dst/src is NULL");
    if (n <= 0) return IMS_OK;
    hipLaunchKernelGGL(k_image_add, dim3(grid_for_pool(n)), dim3(256), 0, (hipStream_t)stream, dst, src, n);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_paint_cosmic_rays(double* image_dev, int32_t nx, int32_t ny, const ims_cr_span_t* spans_dev, int64_t n_spans,
                          const double* values_dev, int64_t n_values, const ims_cr_hit_t* hits_dev, const int64_t* layer_first,
                          int32_t n_layers, void* stream)
{
    if (n_layers < 0 || (n_layers > 0 && !layer_first)) return set_err(IMS_ERR_ARG, "cosmic rays: bad layer list");
    if (n_layers == 0 || layer_first[n_layers] == 0) return IMS_OK;
    if (!image_dev || !spans_dev || !values_dev || !hits_dev) return set_err(IMS_ERR_ARG, "cosmic rays: image / spans / values / hits is NULL");
    if (nx < 1 || ny < 1 || n_spans < 1 || n_spans > 0x7fffffffLL || n_values < 1)
        return set_err(IMS_ERR_ARG, "cosmic rays: empty image or catalog");
    if (layer_first[0] != 0) return set_err(IMS_ERR_ARG, "cosmic rays: layer_first[0] must be 0");
    for (int32_t l = 0; l < n_layers; ++l)
        if (layer_first[l + 1] < layer_first[l] || layer_first[l + 1] - layer_first[l] > 0x7fffffffLL)
            return set_err(IMS_ERR_ARG, "cosmic rays: layer_first must be non-decreasing");
    hipStream_t st = (hipStream_t)stream;
    for (int32_t l = 0; l < n_layers; ++l) {
        const int64_t n = layer_first[l + 1] - layer_first[l];
        if (n == 0) continue;
        hipLaunchKernelGGL(k_paint_cosmic_rays, dim3((unsigned)n), dim3(64), 0, st, image_dev, nx, ny, spans_dev, n_spans, values_dev,
                           n_values, hits_dev + layer_first[l]);
    }
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

int ims_image_to_float(const double* src, float* dst, int64_t n, void* stream)
{
    if (!dst || !src) return set_err(IMS_ERR_ARG, "dst/src is NULL");
    if (n <= 0) return IMS_OK;
    hipLaunchKernelGGL(k_image_to_float, dim3(grid_for_pool(n)), dim3(256), 0, (hipStream_t)stream, src, dst, n);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

}  // extern "C"
