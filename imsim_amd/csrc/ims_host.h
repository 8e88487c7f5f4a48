// ims_host.h -- section of the one translation unit (imsim_hip.hip): the library's process-wide host state and the helpers
// every other section uses.  Included first, after the device headers and ims_libs.h.
//
// State: g_err, g_tune, g_timing, g_events, g_events_used, g_state_mutex, g_margin, g_fft_mutex, g_fft_plans (all below).
// Helpers: tuning_defaults, set_err, hip_err, HIP_TRY, LaunchTimer, check_params, grid_for_segments, grid_for_pool, with_nv.
// Measurement builds: IMS_PROBE (ims_probe_read), IMS_HIST (g_hist, ims_hist_read), IMS_EXTRA_LAUNCHES (k_nop).
// Entry points: ims_abi_version, ims_tuning_defaults, ims_get_tuning, ims_set_tuning, ims_last_error, ims_device_count,
// ims_device_info, ims_enable_timing, ims_last_kernel_ms, ims_struct_size.
#pragma once

// Which of its equivalent kernel forms the library launches is decided by ONE explicit block of settings (ims_tuning_t,
// include/imsim_hip.h) that the caller may replace with ims_set_tuning -- never by the caller's environment: the library itself
// reads no environment variable except the file names of the libraries it looks up at run time (csrc/ims_libs.h).
static ims_tuning_t tuning_defaults()
{
    ims_tuning_t t;
    t.chain_kernels = 1; t.layout_kernels = 1; t.psf_screens_kernel = 1; t.photon_lds = -1;
    t.round_compact = 1; t.init_tiles = 1; t.upd_dpp = 1; t.joint_lists = 1;
    t.upd_dpp_max = 128; t.joint_list_min = 1024; t.active_fraction = 0.25;
    t.round_two_segments = 0; t.joint_fine_marks = 1; t.joint_search_lists = 1; t.pad = 0;
    return t;
}

// ---------------- process-wide mutable host state ----------------
// The host objects of the library that outlive a call.  Those at namespace scope are declared here, with what guards them.
// Six stay function-local, where they are initialised at first use (and, for `rings`, where their element type is) -- the two
// plan functions in ims_plan_run.h, fft_inverse_impl in ims_fft_branch.h:
//   plan_event: `evs`, the library events of RECORD / WAIT items by number                      -- under g_state_mutex
//   ims_plans_run_joint: `rings`, per device the ring of joint tables and its cursor            -- under g_state_mutex: the choice
//     of an entry and its `busy` flag (set there, cleared by the call's Undo under the lock again); the entry's buffers are
//     grown and its event recorded by the one call that holds it busy, outside the lock
//   fft_inverse_impl: `asked`, how often a (size, batch, stream) came                           -- under g_fft_mutex
//   fft_inverse_impl: `exec_mutex`, which keeps set-stream + execute of a plan from interleaving between host threads
//   ims_libs::fft() / ims_libs::rccl() (ims_libs.h): the entry-point tables `f` / `r` with `tried` -- each under its own `m`
// (A plan's own events and buffers live in its ims_planner::Plan, owned by the caller's handle: not process-wide.)
static thread_local char g_err[512] = "";  // ims_last_error: one per host thread, no lock
// read by every launch without a lock, written by ims_set_tuning under g_state_mutex
static ims_tuning_t g_tune = tuning_defaults();

// Timing of the dominant kernel: every launch of the selected entry point between ims_enable_timing(which)
// and the query is bracketed by a hipEvent pair on the launch stream (which: 1 = ims_shoot_accumulate,
// 2 = ims_shoot_ops_photons, 3 = ims_fft_kspace_fill).
static int g_timing = 0;
static std::vector<hipEvent_t> g_events;   // pairs
static size_t g_events_used = 0;
// g_state_mutex: the tables may be reached from several host threads (focal plane: one per CCD in flight).  It guards g_events
// and g_events_used in LaunchTimer, g_margin, the writes of g_tune (and ims_get_tuning's copy), plan_event's `evs` and
// ims_plans_run_joint's `rings`.  NOT under it: g_timing anywhere; g_events_used and g_events in ims_enable_timing and
// ims_last_kernel_ms (plain writes and reads); the launches' reads of g_tune.
static std::mutex g_state_mutex;

// the list of the photons a lazy_static launch sets aside: one buffer per (device, stream), sized for every photon of the launch
// (launches on a stream run in order, so the next launch finds the second pass of the one before through with it)
struct MarginBuf { double* list = nullptr; int32_t* count = nullptr; unsigned char* wave_count = nullptr; int64_t waves_cap = 0; uint32_t cap = 0; };
static std::map<std::pair<int, void*>, MarginBuf> g_margin;      // under g_state_mutex (ims_shoot_accumulate)

// the hipFFT plans per (size, transforms per plan, stream), under g_fft_mutex (ims_fft_branch.h: fft_plan_get)
static std::mutex g_fft_mutex;
static std::map<std::tuple<int32_t, int64_t, void*>, hipfftHandle> g_fft_plans;

static int set_err(int code, const char* msg)
{
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}
static int hip_err(hipError_t e, const char* what)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return IMS_ERR_HIP;
}
#define HIP_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_err(e_, #call); } while (0)

struct LaunchTimer {
    hipStream_t st;
    size_t slot;
    bool on;
    LaunchTimer(hipStream_t s, int which) : st(s), slot(0), on(g_timing == which)
    {
        if (on) {
            hipEvent_t first;
            {
                std::lock_guard<std::mutex> lock(g_state_mutex);
                if (g_events_used + 2 > g_events.size()) {
                    hipEvent_t a, b;
                    (void)hipEventCreate(&a); (void)hipEventCreate(&b);
                    g_events.push_back(a); g_events.push_back(b);
                }
                slot = g_events_used;
                g_events_used += 2;
                first = g_events[slot];
                second = g_events[slot + 1];
            }
            (void)hipEventRecord(first, st);
        }
    }
    ~LaunchTimer() { if (on) (void)hipEventRecord(second, st); }
    hipEvent_t second;
};

// -DIMS_PROBE (measurement builds only, tools/dbg/round_probe.py): the stamps of ims_photon.h's PROBE / PROBE_WG, copied out
#ifdef IMS_PROBE
extern "C" int ims_probe_read(unsigned long long* out32, unsigned long long* wg512)
{
    if (wg512 && hipMemcpyFromSymbol(wg512, HIP_SYMBOL(ims::g_probe_wg), 512 * sizeof(unsigned long long)) != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out32, HIP_SYMBOL(ims::g_probe), 32 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
// -DIMS_HIST (measurement builds only, tools/dbg/c5_tile_hist.py): what a listed tile of a joint round holds and costs -- per
// number of charged cells in the update's 23 x 23 halo (bins 0 .. 62, 63 = more): tiles, 10-ns ticks from the tile's entry to
// its last store (thread 0), charged cells inside the tile itself
#ifdef IMS_HIST
__device__ unsigned long long g_hist[3][64];
extern "C" int ims_hist_read(unsigned long long* out192, int reset)
{
    if (hipMemcpyFromSymbol(out192, HIP_SYMBOL(g_hist), 192 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        static unsigned long long zero[192];
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_hist), zero, sizeof(zero)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

#ifdef IMS_EXTRA_LAUNCHES
__global__ void k_nop(int* p) { if (p) *p = 0; }      // (measurement builds: empty launches on the joint stream -- what a kernel boundary costs a round)
#endif

constexpr int N_XCD = 8;           // block b runs on XCD b % 8: the photon kernels deal segments to the XCDs in contiguous ranges

static int check_params(const ims_render_params_t* p)
{
    if (!p) return set_err(IMS_ERR_ARG, "params is NULL");
    if (p->n_objects < 0 || p->n_segments < 0) return set_err(IMS_ERR_ARG, "negative object/segment count");
    if (p->n_objects > 0 && (!p->objects || !p->seg_prefix)) return set_err(IMS_ERR_ARG, "objects/seg_prefix is NULL");
    if (p->seg_size != 256) return set_err(IMS_ERR_ARG, "seg_size must be 256 (one photon per thread of a 256-thread workgroup)");
    if (p->n_psf < 0 || p->n_psf > IMS_MAX_PSF) return set_err(IMS_ERR_ARG, "n_psf out of range");
    if (p->n_ops < 0 || p->n_ops > IMS_MAX_OPS) return set_err(IMS_ERR_ARG, "n_ops out of range");
    for (int k = 0; k < p->n_psf; ++k)
        if (p->psf[k].kind == IMS_PSF_SCREENS && !p->atm) return set_err(IMS_ERR_ARG, "phase-screen PSF without atmosphere descriptor");
    int n_optical = 0;
    for (int k = 0; k < p->n_psf; ++k) {
        if (p->psf[k].kind != IMS_PSF_OPTICAL_SCREEN) continue;
        if (!p->atm) return set_err(IMS_ERR_ARG, "optical phase screen without its descriptor (atm must point to an ims_atmosphere_optical_t)");
        if (p->psf[k].chrom_alpha != 0.0) return set_err(IMS_ERR_ARG, "the optical phase screen is achromatic (chrom_alpha must be 0)");
        if (++n_optical > 1) return set_err(IMS_ERR_ARG, "more than one optical phase screen");
        // the phase screens address their deviates by their place among the components that are not the optical screen, the
        // pre-pass (ims_screen_prepass) by their place in the list: the same only while the optical screen comes after them
        for (int c = k + 1; c < p->n_psf; ++c)
            if (p->psf[c].kind == IMS_PSF_SCREENS)
                return set_err(IMS_ERR_ARG, "the optical phase screen must come after the IMS_PSF_SCREENS component (the order of AtmosphericPSF.getPSF)");
    }
    for (int k = 0; k < p->n_ops; ++k) {
        const int kind = p->ops[k].kind;
        if ((kind == IMS_OP_RUBIN_OPTICS || kind == IMS_OP_RUBIN_DIFFRACTION || kind == IMS_OP_RUBIN_DIFFRACTION_OPTICS) && !p->optics)
            return set_err(IMS_ERR_ARG, "Rubin optics op without optics descriptor");
    }
    return IMS_OK;
}

static unsigned grid_for_segments(int64_t n_segments)
{
    const int64_t per = (n_segments + N_XCD - 1) / N_XCD;
    return (unsigned)(per * N_XCD);
}

static unsigned grid_for_pool(int64_t n)
{
    int64_t blocks = (n + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

// f(std::integral_constant<int, NV>) with the vertices per pixel edge as the sensor kernels' template argument: 4, 8, or 0 for
// the forms that loop over any count
template <class F>
static void with_nv(int num_vertices, F&& f)
{
    if (num_vertices == 4) f(std::integral_constant<int, 4>{});
    else if (num_vertices == 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 0>{});
}

extern "C" {

int ims_abi_version(void) { return IMS_ABI_VERSION; }

int ims_tuning_defaults(ims_tuning_t* out)
{
    if (!out) return set_err(IMS_ERR_ARG, "out is NULL");
    *out = tuning_defaults();
    return IMS_OK;
}
int ims_get_tuning(ims_tuning_t* out)
{
    if (!out) return set_err(IMS_ERR_ARG, "out is NULL");
    std::lock_guard<std::mutex> lock(g_state_mutex);
    *out = g_tune;
    return IMS_OK;
}
int ims_set_tuning(const ims_tuning_t* t)
{
    if (!t) return set_err(IMS_ERR_ARG, "tuning is NULL");
    if (t->photon_lds > 65536 - 4096) return set_err(IMS_ERR_ARG, "tuning: photon_lds beyond what a workgroup may ask for");
    if (t->upd_dpp_max < 0 || t->joint_list_min < 0 || !(t->active_fraction > 0.0) || t->active_fraction > 1.0)
        return set_err(IMS_ERR_ARG, "tuning: upd_dpp_max / joint_list_min / active_fraction out of range");
    std::lock_guard<std::mutex> lock(g_state_mutex);
    g_tune = *t;
    return IMS_OK;
}
const char* ims_last_error(void) { return g_err; }

int ims_device_count(int* count)
{
    if (!count) return set_err(IMS_ERR_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return hip_err(e, "hipGetDeviceCount"); }
    *count = n;
    return IMS_OK;
}

int ims_device_info(int device, int* n_cu, int* n_xcd, int64_t* lds_bytes, int64_t* hbm_bytes)
{
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (n_xcd) *n_xcd = N_XCD;
    if (lds_bytes) *lds_bytes = (int64_t)prop.sharedMemPerMultiprocessor;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    return IMS_OK;
}

int ims_enable_timing(int which) { g_timing = which; g_events_used = 0; return IMS_OK; }

int ims_last_kernel_ms(float* ms, int* n_launches)
{
    if (!ms) return set_err(IMS_ERR_ARG, "ms is NULL");
    if (g_events_used == 0) return set_err(IMS_ERR_ARG, "no timed launch recorded");
    float total = 0.0f;
    for (size_t k = 0; k < g_events_used; k += 2) {
        float t = 0.0f;
        HIP_TRY(hipEventSynchronize(g_events[k + 1]));
        HIP_TRY(hipEventElapsedTime(&t, g_events[k], g_events[k + 1]));
        total += t;
    }
    *ms = total;
    if (n_launches) *n_launches = (int)(g_events_used / 2);
    g_events_used = 0;
    return IMS_OK;
}

int ims_struct_size(int which)
{
    switch (which) {
    case 0: return (int)sizeof(ims_object_t);
    case 1: return (int)sizeof(ims_radial_tables_t);
    case 2: return (int)sizeof(ims_lin_tables_t);
    case 3: return (int)sizeof(ims_psf_component_t);
    case 4: return (int)sizeof(ims_op_t);
    case 5: return (int)sizeof(ims_surface_t);
    case 6: return (int)sizeof(ims_tansip_t);
    case 7: return (int)sizeof(ims_optics_t);
    case 8: return (int)sizeof(ims_bf_slot_t);
    case 9: return (int)sizeof(ims_sensor_t);
    case 10: return (int)sizeof(ims_photons_t);
    case 11: return (int)sizeof(ims_render_params_t);
    case 12: return (int)sizeof(ims_plan_item_t);
    case 13: return (int)sizeof(ims_atmosphere_t);
    case 14: return (int)sizeof(ims_fft_object_t);
    case 15: return (int)sizeof(ims_fft_params_t);
    case 16: return (int)sizeof(ims_readout_t);
    case 17: return (int)sizeof(ims_chain_t);
    case 18: return (int)sizeof(ims_catalog_t);
    case 19: return (int)sizeof(ims_object_meta_t);
    case 20: return (int)sizeof(ims_plan_input_t);
    case 21: return (int)sizeof(ims_plan_sizes_t);
    case 22: return (int)sizeof(ims_tuning_t);
    case 23: return (int)sizeof(ims_opd_t);
    case 24: return (int)sizeof(ims_optics_perturbed_t);
    case 25: return (int)sizeof(ims_perturbation_t);
    case 26: return (int)sizeof(ims_cr_span_t);
    case 27: return (int)sizeof(ims_cr_hit_t);
    case 28: return (int)sizeof(ims_optical_screen_t);
    case 29: return (int)sizeof(ims_atmosphere_optical_t);
    case 30: return (int)sizeof(ims_psf_image_t);
    }
    return -1;
}

}  // extern "C"
