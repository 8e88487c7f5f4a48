// ims_plan_run.h -- section of the one translation unit (imsim_hip.hip): running launch plans.
//
// Plan items (ims_run_plan; the rounds of several chain classes side by side: run_rounds), then the LSST_Image launch planner's
// binding to memory, upload and run (ims_plan.h, included below, builds the plan), and the CCDs of a visit run jointly.
// Needs the photon and boundary entry points of imsim_hip.hip and ims_gather_rows of ims_table.h.
// Kernel: k_scatter_add.  Entry points: ims_run_plan, ims_plan_lsst_image .. ims_plan_add_realized, ims_plans_run_joint.
#pragma once

extern "C" {

// library events of RECORD / WAIT items (one process per GPU)
static int plan_event(int number, hipEvent_t* out)
{
    static std::unordered_map<int, hipEvent_t> evs;
    if (number < 0 || number > 65535) return set_err(IMS_ERR_ARG, "plan event number out of range");
    std::lock_guard<std::mutex> lock(g_state_mutex);
    auto it = evs.find(number);
    if (it == evs.end()) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        it = evs.emplace(number, e).first;
    }
    *out = it->second;
    return IMS_OK;
}

// objects of a table sorted by photon count (descending) that have more than `threshold` photons
static int32_t count_above(const int64_t* n_phot, int32_t n, int64_t threshold)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) / 2;
        if (n_phot[mid] > threshold) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// tiles of the chain's regions that go on after round `round` (the objects with photons beyond it)
static int64_t tiles_going_on(const ims_chain_t& ch, int32_t round, int32_t nrecalc)
{
    const int32_t n_cont = count_above(ch.n_phot, ch.n_objects, (int64_t)(round + 1) * nrecalc);
    return n_cont > 0 ? ch.tile_prefix_host[n_cont] : 0;
}

// IMS_PLAN_ROUNDS: the rounds of several chain classes, enqueued round by round so that every chain advances at the same pace
static int run_rounds(const ims_chain_t* chains, int32_t n_chains, const ims_sensor_t* sensor_dev, const ims_sensor_t* sensor_host,
                      unsigned char* changed_dev, void* const* streams, int32_t n_streams)
{
    if (!chains || n_chains < 0 || n_chains > IMS_MAX_CHAINS) return set_err(IMS_ERR_ARG, "chains is NULL or too many chains");
    int32_t max_rounds = 0;
    for (int32_t c = 0; c < n_chains; ++c) {
        const ims_chain_t& ch = chains[c];
        if (!ch.params || !ch.pool || !ch.pool_start || !ch.n_phot || !ch.tile_prefix || !ch.tile_prefix_host)
            return set_err(IMS_ERR_ARG, "chain: NULL pointer");
        if (ch.stream < 0 || ch.stream >= n_streams) return set_err(IMS_ERR_ARG, "chain stream index out of range");
        if (ch.nrecalc <= 0 || ch.n_rounds < 0 || ch.n_objects < 0 || ch.n_objects > ch.params->n_objects)
            return set_err(IMS_ERR_ARG, "chain: nrecalc / n_rounds / n_objects out of range");
        if (ch.n_edges < 0 || ch.n_edges > IMS_MAX_CHAIN_EDGES) return set_err(IMS_ERR_ARG, "chain: too many edges");
        for (int32_t k = 1; k < ch.n_objects; ++k)
            if (ch.n_phot[k] > ch.n_phot[k - 1]) return set_err(IMS_ERR_ARG, "chain: objects must be sorted by photon count, brightest first");
        if (ch.n_rounds > max_rounds) max_rounds = ch.n_rounds;
    }
    for (int32_t r = 0; r < max_rounds; ++r) {
        for (int32_t c = 0; c < n_chains; ++c) {
            const ims_chain_t& ch = chains[c];
            if (r >= ch.n_rounds) continue;
            void* st = streams[ch.stream];
            for (int32_t j = 1; j < ch.n_edges; ++j)
                if (ch.edges[j] == r) {
                    hipEvent_t e;
                    const int rc = plan_event(ch.ev_base + j, &e);
                    if (rc) return rc;
                    HIP_TRY(hipStreamWaitEvent((hipStream_t)st, e, 0));
                }
            const int32_t n_act = count_above(ch.n_phot, ch.n_objects, (int64_t)r * ch.nrecalc);
            if (n_act == 0) continue;
            const uint32_t tag = ch.use_tags ? (uint32_t)(r % 255 + 1) : 0u;       // marks the tiles this round's charge lands in
            // (the varying fields are set in a copy that is only read on the host: the launch takes the compact argument block)
            ims_render_params_t P = *ch.params;
            P.bf_tag = tag;
            P.bf_slot_shift = 0u;
            int rc = accumulate_round_compact(&P, ch.pool, ch.pool_start, r, ch.nrecalc, n_act, sensor_host ? sensor_host->num_vertices : 0, st);
            if (rc) return rc;
            const int32_t n_cont = count_above(ch.n_phot, ch.n_objects, (int64_t)(r + 1) * ch.nrecalc);
            if (n_cont > 0) {
                rc = ims_sensor_update_distortions(sensor_dev, sensor_host, ch.first_slot, n_cont, ch.tile_prefix,
                                                   ch.tile_prefix_host[n_cont], changed_dev, tag, st);
                if (rc) return rc;
            }
        }
    }
    return IMS_OK;
}

int ims_run_plan(const ims_plan_item_t* items, int64_t n_items, const ims_sensor_t* sensor_dev,
                 const ims_sensor_t* sensor_host, unsigned char* changed_dev, void* const* streams, int32_t n_streams)
{
    if (!items && n_items > 0) return set_err(IMS_ERR_ARG, "items is NULL");
    if (!streams || n_streams <= 0) return set_err(IMS_ERR_ARG, "streams is NULL");
    for (int64_t k = 0; k < n_items; ++k)
        if (items[k].stream < 0 || items[k].stream >= n_streams) return set_err(IMS_ERR_ARG, "plan item stream index out of range");
    for (int64_t k = 0; k < n_items; ++k) {
        const ims_plan_item_t& it = items[k];
        void* st = streams[it.stream];
        int rc = IMS_OK;
        switch (it.kind) {
        case IMS_PLAN_RENDER:     rc = ims_shoot_accumulate(it.params, st); break;
        case IMS_PLAN_SHOOT_POOL: rc = ims_shoot_ops_photons(it.params, it.aux, it.pool, st); break;
        case IMS_PLAN_ACC_POOL:   rc = ims_accumulate_segments(it.params, it.pool, it.aux, sensor_host ? sensor_host->num_vertices : 0, st); break;
        case IMS_PLAN_UPDATE:     rc = ims_sensor_update_distortions(sensor_dev, sensor_host, it.first_slot, it.n_slots, it.aux,
                                                                     it.n_tiles, changed_dev, it.tag, st); break;
        case IMS_PLAN_INIT:       rc = ims_sensor_init_boundaries(sensor_dev, sensor_host, it.first_slot, it.n_slots, it.aux, it.n_tiles, st); break;
        case IMS_PLAN_ROUNDS:     rc = run_rounds((const ims_chain_t*)it.aux2, it.n_slots, sensor_dev, sensor_host, changed_dev, streams,
                                                  n_streams); break;
        case IMS_PLAN_RECORD:
        case IMS_PLAN_WAIT: {
            hipEvent_t e;
            rc = plan_event(it.n_slots, &e);
            if (rc) return rc;
            if (it.kind == IMS_PLAN_RECORD) HIP_TRY(hipEventRecord(e, (hipStream_t)st));
            else HIP_TRY(hipStreamWaitEvent((hipStream_t)st, e, 0));
            break; }
        default: return set_err(IMS_ERR_ARG, "unknown plan item kind");
        }
        if (rc) return rc;
    }
    return IMS_OK;
}

// ---- LSST_Image launch planner (csrc/ims_plan.h builds the plan; here: binding to memory, upload, run) ----
}  // extern "C"
#include "ims_plan.h"

__global__ __launch_bounds__(256) void k_scatter_add(const int64_t* __restrict__ where, const double* __restrict__ src,
                                                     double* __restrict__ dst, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && src[i] != 0.0) unsafeAtomicAdd(dst + where[i], src[i]);
}

extern "C" {

int ims_plan_lsst_image(const ims_plan_input_t* in, void** plan_out, ims_plan_sizes_t* sizes)
{
    if (!in || !plan_out || !sizes) return set_err(IMS_ERR_ARG, "NULL argument");
    ims_planner::Plan* pl = new ims_planner::Plan();
    pl->in = *in;
    const int rc = ims_planner::build(*pl);
    if (rc) { delete pl; return rc; }
    // the plan keeps nothing of the caller's arrays
    pl->in.row = nullptr; pl->in.n_phot = nullptr; pl->in.stamp = nullptr; pl->in.faint = nullptr;
    *sizes = pl->sizes;
    *plan_out = pl;
    return IMS_OK;
}

int ims_plan_destroy(void* plan)
{
    ims_planner::Plan* pl = (ims_planner::Plan*)plan;
    if (!pl) return IMS_OK;
    for (hipEvent_t e : pl->events) (void)hipEventDestroy(e);
    for (hipEvent_t e : pl->d_events) (void)hipEventDestroy(e);
    delete pl;
    return IMS_OK;
}

int ims_plan_bind(void* plan, const ims_render_params_t* base, void* arena_host, void* arena_dev, void* rows_dev,
                  const ims_object_t* master_dev, double* pool_dev, double* realized_dev)
{
    using namespace ims_planner;
    Plan* pl = (Plan*)plan;
    if (!pl || !base || !arena_host || !arena_dev || !rows_dev || !master_dev) return set_err(IMS_ERR_ARG, "NULL argument");
    if (pl->sizes.pool_photons > 0 && !pool_dev) return set_err(IMS_ERR_ARG, "pool_dev is NULL");
    if (pl->sizes.realized_count > 0 && !realized_dev) return set_err(IMS_ERR_ARG, "realized_dev is NULL");
    pl->arena_host = (uint8_t*)arena_host; pl->arena_dev = (uint8_t*)arena_dev; pl->rows_dev = (uint8_t*)rows_dev;
    pl->master_dev = master_dev; pl->pool_dev = pool_dev; pl->realized_dev = realized_dev;
    std::memcpy(pl->arena_host, pl->arena.data(), pl->arena.size());
    auto dev = [&](int64_t off) { return off < 0 ? (uint8_t*)nullptr : pl->arena_dev + off; };
    for (Launch& L : pl->launches) {
        L.P = *base;
        L.P.objects = (const ims_object_t*)(pl->rows_dev + L.rows_off);
        L.P.n_objects = L.n;
        L.P.seg_prefix = (const int64_t*)dev(L.off_prefix);
        L.P.n_segments = L.n_segments;
        L.P.seg_object = (const int32_t*)dev(L.off_segobj);
        L.P.realized_flux = (L.realized_off >= 0) ? pl->realized_dev + L.realized_off : nullptr;
        L.P.bf_tag = 0; L.P.bf_slot_shift = 0;
        L.P.lazy_static = 0;                 // (set again below for the launches that are fused renders: nothing else may carry it)
    }
    for (Group& g : pl->groups) {
        std::memset(&g.pool, 0, sizeof(g.pool));
        g.pool.n = g.pool_photons;
        g.pool.converted = 1;
        const int64_t np = pl->sizes.pool_photons;
        g.pool.x = pool_dev; g.pool.y = pool_dev ? pool_dev + np : nullptr;
        g.pool.flux = pool_dev ? pool_dev + 2 * np : nullptr; g.pool.dxdz = pool_dev ? pool_dev + 3 * np : nullptr;
        g.chain_structs.assign(g.chains.size(), ims_chain_t());
        for (size_t c = 0; c < g.chains.size(); ++c) {
            const ChainDesc& ch = g.chains[c];
            ims_chain_t& cs = g.chain_structs[c];
            std::memset(&cs, 0, sizeof(cs));
            const Launch& L = pl->launches[ch.launch];
            cs.params = &L.P; cs.pool = &g.pool;

            cs.pool_start = (const int64_t*)dev(L.off_pool);
            cs.n_phot = ch.n_phot.data();
            cs.tile_prefix = (const int64_t*)dev(ch.off_tile_prefix);
            cs.tile_prefix_host = ch.tile_prefix_host.data();
            cs.n_objects = (int32_t)ch.n_phot.size(); cs.first_slot = ch.first_slot; cs.stream = ch.stream; cs.nrecalc = pl->in.nrecalc;
            cs.n_rounds = ch.n_rounds; cs.use_tags = pl->in.use_tags; cs.ev_base = ch.ev_base; cs.n_edges = (int32_t)ch.edges.size();
            for (size_t k = 0; k < ch.edges.size(); ++k) cs.edges[k] = ch.edges[k];
        }
        g.items.assign(g.steps.size(), ims_plan_item_t());
        for (size_t k = 0; k < g.steps.size(); ++k) {
            const Step& s = g.steps[k];
            ims_plan_item_t& it = g.items[k];
            std::memset(&it, 0, sizeof(it));
            it.kind = s.kind; it.stream = s.stream;
            switch (s.kind) {
            case IMS_PLAN_RENDER: pl->launches[s.launch].P.lazy_static = base->lazy_static; it.params = &pl->launches[s.launch].P; break;
            case IMS_PLAN_SHOOT_POOL:
                it.params = &pl->launches[s.launch].P; it.pool = &g.pool; it.aux = (const int64_t*)dev(pl->launches[s.launch].off_pool); break;
            case IMS_PLAN_INIT:
                it.first_slot = s.first_slot; it.n_slots = s.n_slots; it.aux = (const int64_t*)dev(s.off_tile_prefix); it.n_tiles = s.n_tiles; break;
            case IMS_PLAN_RECORD: it.n_slots = s.event; break;
            case IMS_PLAN_WAIT: it.n_slots = s.event; break;
            case IMS_PLAN_ROUNDS: it.n_slots = s.n_chains; it.aux2 = g.chain_structs.data() + s.chain_begin; break;
            default: return set_err(IMS_ERR_ARG, "planner: unexpected step kind");
            }
        }
    }
    pl->bound = true; pl->uploaded = false;
    return IMS_OK;
}

int ims_plan_upload(void* plan, void* stream)
{
    using namespace ims_planner;
    Plan* pl = (Plan*)plan;
    if (!pl || !pl->bound) return set_err(IMS_ERR_ARG, "plan is NULL or not bound");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(pl->arena_dev, pl->arena_host, pl->arena.size(), hipMemcpyHostToDevice, st));
    for (const Launch& L : pl->launches) {
        if (L.n <= 0) continue;
        const int rc = ims_gather_rows(pl->master_dev, (const int64_t*)(pl->arena_dev + L.off_index), (const int64_t*)(pl->arena_dev + L.off_first),
                                       (const int64_t*)(pl->arena_dev + L.off_count), (const int32_t*)(pl->arena_dev + L.off_bf), 0,
                                       (ims_object_t*)(pl->rows_dev + L.rows_off), L.n, stream);
        if (rc) return rc;
    }
    pl->uploaded = true;
    return IMS_OK;
}

static int plan_enqueue(ims_planner::Plan* pl, ims_sensor_t* sensor_dev, ims_sensor_t* sensor_host, ims_bf_slot_t* slots_dev,
                        unsigned char* changed_dev, void* main_stream, void* const* streams, int32_t n_streams, int32_t own_work_queued,
                        bool defer_top = false)
{
    using namespace ims_planner;
    if (!streams || n_streams < 5) return set_err(IMS_ERR_ARG, "streams: five plan streams by role are required");
    bool any_slots = false;
    for (const Group& g : pl->groups) any_slots = any_slots || g.n_slots > 0;
    if (any_slots && (!sensor_dev || !sensor_host || !slots_dev || !changed_dev || !sensor_host->bf_slots))
        return set_err(IMS_ERR_ARG, "sensor / slot table / changed is NULL");
    // the rounds of the top chain can be left to a joint run when the plan is ONE group of regions (a later group rewrites the
    // slot table behind everything queued) in the form the joint kernels take: 4 vertices per edge, qdist 3, regions in place
    pl->deferred = false;
    bool defer = defer_top && pl->groups.size() == 1 && pl->groups[0].n_slots > 0 && !pl->groups[0].chain_structs.empty() &&
                 sensor_host->num_vertices == IT_NV && sensor_host->qdist == 3;
    if (defer)
        for (const ims_chain_t& cs : pl->groups[0].chain_structs)
            defer = defer && cs.first_slot > 0;
    // distinct streams
    std::vector<hipStream_t> uniq;
    for (int k = 0; k < n_streams; ++k)
        if (std::find(uniq.begin(), uniq.end(), (hipStream_t)streams[k]) == uniq.end()) uniq.push_back((hipStream_t)streams[k]);
    const size_t need = 2 + 2 * uniq.size();
    while (pl->events.size() < need) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        pl->events.push_back(e);
    }
    hipStream_t main = (hipStream_t)main_stream, chain = (hipStream_t)streams[ROLE_CHAIN];
    if (pl->realized_dev && pl->sizes.realized_count > 0)
        HIP_TRY(hipMemsetAsync(pl->realized_dev, 0, (size_t)pl->sizes.realized_count * sizeof(double), main));
    HIP_TRY(hipEventRecord(pl->events[0], main));
    for (hipStream_t s : uniq) HIP_TRY(hipStreamWaitEvent(s, pl->events[0], 0));
    bool queued = own_work_queued != 0;
    for (size_t gi = 0; gi < pl->groups.size(); ++gi) {
        Group& g = pl->groups[gi];
        if (g.n_slots > 0) {
            const int n0 = pl->in.n_static_slots;
            if (n0 + g.n_slots > pl->in.slot_capacity) return set_err(IMS_ERR_ARG, "too many brighter-fatter slots");
            // The slot table is rewritten by a copy on the chain stream: behind everything this renderer has queued on every
            // stream (a later group's table must not change under the launches of the one before) and ahead of what follows
            if (queued)
                for (size_t k = 0; k < uniq.size(); ++k)
                    if (uniq[k] != chain) {
                        HIP_TRY(hipEventRecord(pl->events[2 + k], uniq[k]));
                        HIP_TRY(hipStreamWaitEvent(chain, pl->events[2 + k], 0));
                    }
            HIP_TRY(hipMemcpyAsync(slots_dev + n0, pl->arena_host + g.off_slots, (size_t)g.n_slots * sizeof(ims_bf_slot_t),
                                   hipMemcpyHostToDevice, chain));
            HIP_TRY(hipMemcpyAsync(&sensor_dev->n_bf_slots, pl->arena_host + pl->off_nslots[gi], sizeof(int32_t), hipMemcpyHostToDevice, chain));
            HIP_TRY(hipEventRecord(pl->events[1], chain));
            for (hipStream_t s : uniq) if (s != chain) HIP_TRY(hipStreamWaitEvent(s, pl->events[1], 0));
            std::memcpy((ims_bf_slot_t*)(uintptr_t)sensor_host->bf_slots + n0, pl->arena_host + g.off_slots, (size_t)g.n_slots * sizeof(ims_bf_slot_t));
            sensor_host->n_bf_slots = n0 + g.n_slots;
        }
        if (defer) {
            // without the rounds item: the rounds of ALL chain classes are left to joint runs
            std::vector<ims_plan_item_t> items;
            for (const ims_plan_item_t& it : g.items)
                if (it.kind != IMS_PLAN_ROUNDS) items.push_back(it);
            const int rc = ims_run_plan(items.data(), (int64_t)items.size(), sensor_dev, sensor_host, changed_dev, streams, n_streams);
            if (rc) return rc;
        } else {
            const int rc = ims_run_plan(g.items.data(), (int64_t)g.items.size(), sensor_dev, sensor_host, changed_dev, streams, n_streams);
            if (rc) return rc;
        }
        queued = true;
    }
    if (defer_top) {
        // no join yet (ims_plan_join): where this plan's work ends on every stream is recorded NOW -- on streams shared by role the
        // next CCD's work follows, and a join must not wait for that
        for (size_t k = 0; k < uniq.size(); ++k) HIP_TRY(hipEventRecord(pl->events[2 + uniq.size() + k], uniq[k]));
        pl->unjoined = (int)uniq.size();
        pl->deferred = defer;
        pl->left = defer ? ((1u << pl->groups[0].chain_structs.size()) - 1u) : 0u;
        pl->d_done_used = 0;
        pl->d_sensor_dev = sensor_dev; pl->d_sensor_host = sensor_host; pl->d_changed = changed_dev; pl->d_main = main_stream;
        pl->d_streams.assign(streams, streams + n_streams);
        return IMS_OK;
    }
    for (size_t k = 0; k < uniq.size(); ++k) {
        HIP_TRY(hipEventRecord(pl->events[2 + uniq.size() + k], uniq[k]));
        HIP_TRY(hipStreamWaitEvent(main, pl->events[2 + uniq.size() + k], 0));
    }
    return IMS_OK;
}

// (Two other forms of this call were built, measured in round 4 and removed in round 5: the whole enqueue captured into a
// hipGraph -- capture + instantiate + launch of a CCD's ~3 000-node plan cost the host 51 ms against 24 ms for enqueueing it, and a
// graph does not run on the caller's streams -- and one plan's rounds through the joint runner with its tile lists -- a fourth
// dependent launch per round on a chain of 185 rounds: C3 24.2 -> 25.2 ms without lists, 33 ms with them.)
int ims_plan_run(void* plan, ims_sensor_t* sensor_dev, ims_sensor_t* sensor_host, ims_bf_slot_t* slots_dev, unsigned char* changed_dev,
                 void* main_stream, void* const* streams, int32_t n_streams, int32_t own_work_queued)
{
    using namespace ims_planner;
    Plan* pl = (Plan*)plan;
    if (!pl || !pl->uploaded) return set_err(IMS_ERR_ARG, "plan is NULL or not uploaded");
    return plan_enqueue(pl, sensor_dev, sensor_host, slots_dev, changed_dev, main_stream, streams, n_streams, own_work_queued);
}

int ims_plan_join(void* plan, void* stream)
{
    using namespace ims_planner;
    Plan* pl = (Plan*)plan;
    if (!pl) return set_err(IMS_ERR_ARG, "plan is NULL");
    if (pl->deferred) return set_err(IMS_ERR_ARG, "ims_plan_join: the rounds left by ims_plan_run_deferred have not been run (ims_plans_run_joint)");
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < pl->unjoined; ++k) HIP_TRY(hipStreamWaitEvent(st, pl->events[2 + (size_t)pl->unjoined + k], 0));
    for (size_t k = 0; k < pl->d_done_used; ++k) HIP_TRY(hipStreamWaitEvent(st, pl->d_events[4 + k], 0));
    pl->unjoined = 0; pl->d_done_used = 0;
    return IMS_OK;
}

int ims_plan_run_deferred(void* plan, ims_sensor_t* sensor_dev, ims_sensor_t* sensor_host, ims_bf_slot_t* slots_dev, unsigned char* changed_dev,
                          void* main_stream, void* const* streams, int32_t n_streams, int32_t own_work_queued, int32_t* deferred)
{
    using namespace ims_planner;
    Plan* pl = (Plan*)plan;
    if (!pl || !pl->uploaded) return set_err(IMS_ERR_ARG, "plan is NULL or not uploaded");
    if (!deferred) return set_err(IMS_ERR_ARG, "deferred is NULL");
    const int rc = plan_enqueue(pl, sensor_dev, sensor_host, slots_dev, changed_dev, main_stream, streams, n_streams, own_work_queued, true);
    *deferred = (rc == IMS_OK && pl->deferred) ? (int32_t)pl->groups[0].chain_structs.size() : 0;
    return rc;
}

int ims_plans_run_joint(void* const* plans, int32_t n_plans, void* joint_stream, int32_t first_chain, int32_t n_chains)
{
    using namespace ims_planner;
    if (n_plans < 0 || (n_plans > 0 && !plans)) return set_err(IMS_ERR_ARG, "plans is NULL");
    if (first_chain < 0 || n_chains < 1) return set_err(IMS_ERR_ARG, "joint run: chain range");
    struct Act { Plan* pl; const ims_chain_t* ch; int chain; hipEvent_t done; };
    std::vector<Act> act;
    hipStream_t js = (hipStream_t)joint_stream;
    // what an error return has to undo: the done events handed out below (a plan's join must not wait for a record that
    // never comes) and the ring entry held while this call enqueues (its event is recorded all the same: launches that
    // did go out read the entry's tables)
    struct Undo {
        std::vector<Plan*> counted; bool* busy = nullptr; hipEvent_t table_event = nullptr; hipStream_t js = nullptr; bool ok = false;
        ~Undo() {
            if (!ok) for (Plan* p : counted) if (p->d_done_used > 0) --p->d_done_used;
            if (busy) {
                if (!ok && table_event) (void)hipEventRecord(table_event, js);
                std::lock_guard<std::mutex> lock(g_state_mutex);
                *busy = false;
            }
        }
    } undo;
    undo.js = js;
    for (int32_t k = 0; k < n_plans; ++k) {
        Plan* pl = (Plan*)plans[k];
        if (!pl) return set_err(IMS_ERR_ARG, "plans: NULL entry");
        if (!pl->deferred) continue;                       // ran whole (no bright object, several groups): nothing left to do
        const int nc = (int)pl->groups[0].chain_structs.size();
        bool any = false;
        for (int c = first_chain; c < first_chain + n_chains && c < nc; ++c)
            if (pl->left & (1u << c)) { act.push_back({ pl, &pl->groups[0].chain_structs[c], c, nullptr }); any = true; }
        if (!any) continue;
        // own events: four "chain stream ready", then one per joint run since the last join
        while (pl->d_events.size() < 4 + pl->d_done_used + 1) {
            hipEvent_t e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            pl->d_events.push_back(e);
        }
        const hipEvent_t done = pl->d_events[4 + pl->d_done_used++];
        undo.counted.push_back(pl);
        for (Act& a : act) if (a.pl == pl) a.done = done;
    }
    if (act.empty()) { undo.ok = true; return IMS_OK; }
    if ((int)act.size() > IMS_JOINT_MAX) return set_err(IMS_ERR_ARG, "at most 64 chains per joint run");
    const int32_t nrecalc = act[0].ch->nrecalc, use_tags = act[0].ch->use_tags;
    int32_t max_rounds = 0;
    for (const Act& a : act) {
        const ims_chain_t& ch = *a.ch;
        if (ch.nrecalc != nrecalc || ch.use_tags != use_tags) return set_err(IMS_ERR_ARG, "joint run: the plans differ in nrecalc / tile tags");
        if (!ch.params || !ch.pool || !ch.pool->converted || !ch.pool_start || !ch.params->objects || !ch.params->image)
            return set_err(IMS_ERR_ARG, "joint run: chain without table / pool / image");
        if (ch.n_rounds > max_rounds) max_rounds = ch.n_rounds;
        // the joint stream takes over behind the chain's own stream (the regions' initial state, the first pool slice)
        // (behind the END OF THE CCD'S OWN FRONT on that stream -- the event ims_plan_run_deferred recorded there -- not behind
        // whatever the stream holds by now: the joint run may be enqueued from a second host thread while the fronts of the
        // next batch of CCDs are already being queued on the shared streams, and the chain must not wait for those)
        hipStream_t cs = (hipStream_t)a.pl->d_streams[ch.stream];
        if (cs != js) {
            std::vector<hipStream_t> uniq;
            for (void* st : a.pl->d_streams)
                if (std::find(uniq.begin(), uniq.end(), (hipStream_t)st) == uniq.end()) uniq.push_back((hipStream_t)st);
            const size_t k = (size_t)(std::find(uniq.begin(), uniq.end(), cs) - uniq.begin());
            if ((int)uniq.size() != a.pl->unjoined || k >= uniq.size())
                return set_err(IMS_ERR_ARG, "joint run: the plan was not enqueued by ims_plan_run_deferred on these streams");
            HIP_TRY(hipStreamWaitEvent(js, a.pl->events[2 + uniq.size() + k], 0));
        }
    }
    const int32_t segs = (nrecalc + 255) / 256;
    const long long dpp_max_tiles = g_tune.upd_dpp_max;
    // the per-chain argument blocks in device memory, one table per joint run out of a ring (a table is read until the run's
    // last round: the ring's event says when)
    // active-tile lists (k_build_active_j): on for rounds of more than list_min_tiles tiles; joint_lists = 0: the full sweeps
    const bool lists_on = g_tune.joint_lists != 0;
    const long long list_min_tiles = g_tune.joint_list_min;
    const double list_fraction = g_tune.active_fraction;
    int64_t tiles_max = 0;                                   // round 0 has them all
    for (const Act& a : act) tiles_max += tiles_going_on(*a.ch, 0, nrecalc);
    const bool lists = lists_on && tiles_max > list_min_tiles;
    struct Ring { JointTables* dev; hipEvent_t free_after; bool used; bool busy; unsigned long long* upd; unsigned long long* ref; int* count; int64_t cap;
                  JointRound* rounds_dev; JointRound* rounds_pin; int64_t rounds_cap; unsigned int* words; };
    // one ring per DEVICE (its tables live in that device's memory: one process per GPU is the rule, but a process that holds
    // two devices must not hand the second one the first one's tables)
    static std::map<int, std::pair<std::vector<Ring>, size_t>> rings;
    int device_now = 0;
    HIP_TRY(hipGetDevice(&device_now));
    JointTables* tables_dev = nullptr;
    JointRound* rounds_dev = nullptr;
    JointRound* rounds_pin = nullptr;
    hipEvent_t table_event = nullptr;
    JointLists Ls{ nullptr, nullptr, nullptr };
    unsigned int* words_dev = nullptr;
    // search-side lists (TileLister): the pixel search appends the tiles, no builder launch
    const bool search_lists = lists && g_tune.joint_search_lists != 0;
    {
        std::lock_guard<std::mutex> lock(g_state_mutex);
        std::vector<Ring>& ring = rings[device_now].first;
        size_t& ring_next = rings[device_now].second;
        if (ring.empty()) {
            JointTables* block = nullptr;
            int* counts = nullptr;
            HIP_TRY(hipMalloc((void**)&block, 64 * sizeof(JointTables)));
            HIP_TRY(hipMalloc((void**)&counts, 64 * 4 * sizeof(int)));
            for (int k = 0; k < 64; ++k) {
                Ring r{ block + k, nullptr, false, false, nullptr, nullptr, counts + 4 * k, 0, nullptr, nullptr, 0, nullptr };
                HIP_TRY(hipEventCreateWithFlags(&r.free_after, hipEventDisableTiming));
                ring.push_back(r);
            }
        }
        // an entry another thread is still enqueueing with (its event not yet recorded) is passed over
        size_t tries = 0;
        while (ring[ring_next % ring.size()].busy && tries++ < ring.size()) ++ring_next;
        Ring& r = ring[ring_next++ % ring.size()];
        if (r.busy) return set_err(IMS_ERR_ARG, "joint run: all 64 table entries are being enqueued with");
        if (r.used) HIP_TRY(hipEventSynchronize(r.free_after));
        r.used = true; r.busy = true;
        undo.busy = &r.busy; undo.table_event = r.free_after;
        if (lists && r.cap < tiles_max) {
            // (a growth is a device-wide synchronisation: the capacity is kept and rounded up generously)
            if (r.upd) { HIP_TRY(hipFree(r.upd)); HIP_TRY(hipFree(r.ref)); HIP_TRY(hipFree(r.words)); }
            r.cap = tiles_max + tiles_max / 2 + 65536;
            HIP_TRY(hipMalloc((void**)&r.upd, (size_t)r.cap * sizeof(unsigned long long)));
            HIP_TRY(hipMalloc((void**)&r.ref, (size_t)r.cap * sizeof(unsigned long long)));
            HIP_TRY(hipMalloc((void**)&r.words, (size_t)r.cap * sizeof(unsigned int)));
        }
        if (r.rounds_cap < max_rounds) {
            // the round tables of the run: a page-locked staging buffer and its device copy (grown rarely: capacity kept)
            if (r.rounds_dev) { HIP_TRY(hipFree(r.rounds_dev)); HIP_TRY(hipHostFree(r.rounds_pin)); }
            r.rounds_cap = max_rounds + max_rounds / 2 + 64;
            HIP_TRY(hipMalloc((void**)&r.rounds_dev, (size_t)r.rounds_cap * sizeof(JointRound)));
            HIP_TRY(hipHostMalloc((void**)&r.rounds_pin, (size_t)r.rounds_cap * sizeof(JointRound), hipHostMallocDefault));
        }
        tables_dev = r.dev; table_event = r.free_after;
        Ls.upd = r.upd; Ls.ref = r.ref; Ls.count = r.count;
        words_dev = r.words;
        rounds_dev = r.rounds_dev; rounds_pin = r.rounds_pin;
    }
    if (lists) HIP_TRY(hipMemsetAsync(Ls.count, 0, 4 * sizeof(int), js));
    if (search_lists) HIP_TRY(hipMemsetAsync(words_dev, 0, (size_t)tiles_max * sizeof(unsigned int), js));
    // a chain's tile words: behind those of the chains before it (round 0 lists from all the regions that go on)
    std::vector<int64_t> word_off(act.size() + 1, 0);
    for (size_t k = 0; k < act.size(); ++k) word_off[k + 1] = word_off[k] + tiles_going_on(*act[k].ch, 0, nrecalc);
    bool dpp_ok = true;
    for (size_t k0 = 0; k0 < act.size(); k0 += JOINT_CHUNK) {
        JointChunk Ck;
        std::memset(&Ck, 0, sizeof(Ck));
        for (size_t k = 0; k < (size_t)JOINT_CHUNK; ++k) {
            const Act& a = act[k0 + k < act.size() ? k0 + k : 0];         // entries beyond the last repeat chain 0 (never selected: zero width)
            const ims_chain_t& ch = *a.ch;
            Ck.a[k] = round_args(*ch.params, *ch.pool);
            Ck.a[k].bf_tag = 0; Ck.a[k].bf_slot_shift = 0;                    // (the launch brings the round's tag)
            Ck.pool_start[k] = ch.pool_start;
            Ck.sp[k] = a.pl->d_sensor_dev; Ck.tile_prefix[k] = ch.tile_prefix; Ck.changed[k] = a.pl->d_changed;
            Ck.dl[k] = a.pl->d_sensor_host->bf_dl; Ck.first_slot[k] = ch.first_slot;
            Ck.words[k] = (search_lists && k0 + k < act.size()) ? words_dev + word_off[k0 + k] : nullptr;
            dpp_ok = dpp_ok && a.pl->d_sensor_host->bf_dl != nullptr;
        }
        hipLaunchKernelGGL(k_store_joint_tables, dim3(1), dim3(64), 0, js, Ck, tables_dev, (int)k0);
        HIP_TRY(hipGetLastError());
    }
    // every round's tables (workgroup / tile ends per chain) in one pass on the host, ONE copy to the device; per round the
    // launches then take a pointer
    struct RoundTotals { int64_t wgs, tiles, build_wgs; };
    std::vector<RoundTotals> totals((size_t)max_rounds);
    for (int32_t r = 0; r < max_rounds; ++r) {
        JointRound& R = rounds_pin[r];
        int64_t wgs = 0, tiles = 0, build_wgs = 0;
        for (int k = 0; k < IMS_JOINT_MAX; ++k) {
            int32_t n_act = 0, n_cont = 0;
            int64_t tk = 0;
            if (k < (int)act.size() && r < act[k].ch->n_rounds) {
                const ims_chain_t& ch = *act[k].ch;
                n_act = count_above(ch.n_phot, ch.n_objects, (int64_t)r * nrecalc);
                n_cont = count_above(ch.n_phot, ch.n_objects, (int64_t)(r + 1) * nrecalc);
                tk = tiles_going_on(ch, r, nrecalc);
            }
            tiles += tk;
            build_wgs += (tk + 255) / 256;
            wgs += (int64_t)n_act * segs;
            if (wgs > 0x7fffffffLL || tiles > 0x7fffffffLL) return set_err(IMS_ERR_ARG, "joint run: too many workgroups for one round");
            R.ea.v[k] = (int32_t)wgs; R.eu.v[k] = (int32_t)tiles; R.ns.v[k] = n_cont > 0 ? n_cont : 1;
            R.ewg.v[k] = (int32_t)build_wgs; R.tof.v[k] = (int32_t)tk;
        }
        totals[(size_t)r] = { wgs, tiles, build_wgs };
    }
    if (max_rounds > 0)
        HIP_TRY(hipMemcpyAsync(rounds_dev, rounds_pin, (size_t)max_rounds * sizeof(JointRound), hipMemcpyHostToDevice, js));
    // the round after which a CCD's chains of this run are through (its longest chain)
    std::vector<std::pair<int32_t, hipEvent_t>> done_at;
    for (size_t k = 0; k < act.size(); ++k) {
        bool first_of_plan = true;
        int32_t last = 0;
        for (size_t j = 0; j < act.size(); ++j)
            if (act[j].pl == act[k].pl) { if (j < k) first_of_plan = false; if (act[j].ch->n_rounds > last) last = act[j].ch->n_rounds; }
        if (first_of_plan) done_at.push_back({ last - 1, act[k].done });
    }
    for (int32_t r = 0; r < max_rounds; ++r) {
        for (const Act& a : act) {
            const ims_chain_t& ch = *a.ch;
            if (r >= ch.n_rounds) continue;
            for (int32_t j = 1; j < ch.n_edges; ++j)
                if (ch.edges[j] == r) {
                    hipEvent_t e;
                    const int rc = plan_event(ch.ev_base + j, &e);
                    if (rc) return rc;
                    HIP_TRY(hipStreamWaitEvent(js, e, 0));
                }
        }
        const uint32_t tag = (use_tags || lists) ? (uint32_t)(r % 255 + 1) : 0u;
        const int64_t wgs = totals[(size_t)r].wgs, tiles = totals[(size_t)r].tiles, build_wgs = totals[(size_t)r].build_wgs;
        const JointRound* R = rounds_dev + r;
        const bool list_round = tiles > 0 && lists && tiles > list_min_tiles;
        const int parity_r = r & 1;
        if (wgs > 0) {
            LaunchTimer tm(js, 4);
            const bool sl = search_lists && list_round;
            hipLaunchKernelGGL((k_accumulate_round_j<4, 256>), dim3((unsigned)wgs), dim3(256), 0, js, (const JointAcc*)&tables_dev->acc, R, tag,
                               (int64_t)r * nrecalc, nrecalc, segs, sl ? Ls.upd : (unsigned long long*)nullptr,
                               sl ? Ls.count + 2 * parity_r : (int*)nullptr, (unsigned int)(r + 1));
        }
        if (list_round) {
            // marks -> lists -> the update and the refresh over the listed tiles (a launch of a fraction of the tiles walks them)
            const JointUpd* U = &tables_dev->upd;
            const int parity = r & 1;
            int64_t grid = (int64_t)((double)tiles * list_fraction);
            if (grid < 256 && list_fraction >= 0.05) grid = 256;
            if (grid < 1) grid = 1;
            if (grid > tiles) grid = tiles;
            if (!search_lists)
                hipLaunchKernelGGL(k_build_active_j, dim3((unsigned)build_wgs), dim3(256), 0, js, U, R, tag, Ls, parity, (int)g_tune.joint_fine_marks);
            hipLaunchKernelGGL((k_update_list_j<4, false>), dim3((unsigned)grid), dim3(256), 0, js, U, Ls, parity, tag, search_lists ? 1 : 0);
            hipLaunchKernelGGL(k_refresh_list_j<4>, dim3((unsigned)grid), dim3(256), 0, js, U, Ls, parity, tag, search_lists ? 1 : 0);
        } else if (tiles > 0) {
            const JointUpd* U = &tables_dev->upd;
            const bool dpp = dpp_ok && g_tune.upd_dpp && tiles <= dpp_max_tiles;
            if (dpp) hipLaunchKernelGGL((k_update_distortions_q3_j<4, true>), dim3((unsigned)tiles), dim3(256), 0, js, U, R, tag);
            else hipLaunchKernelGGL((k_update_distortions_q3_j<4, false>), dim3((unsigned)tiles), dim3(256), 0, js, U, R, tag);
            hipLaunchKernelGGL(k_refresh_changed_j<4>, dim3((unsigned)tiles), dim3(256), 0, js, U, R, tag);
        }
#ifdef IMS_EXTRA_LAUNCHES
        for (int xl = 0; xl < IMS_EXTRA_LAUNCHES; ++xl) hipLaunchKernelGGL(k_nop, dim3(1), dim3(64), 0, js, (int*)nullptr);
#endif
        // a CCD's chains of this run are through with the longest of them
        for (const auto& d : done_at)
            if (d.first == r) HIP_TRY(hipEventRecord(d.second, js));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(table_event, js));
    undo.ok = true;
    for (const Act& a : act) {
        a.pl->left &= ~(1u << a.chain);
        if (a.pl->left == 0u) a.pl->deferred = false;
    }
    return IMS_OK;
}

int ims_plan_add_realized(void* plan, double* out_dev, void* stream)
{
    using namespace ims_planner;
    Plan* pl = (Plan*)plan;
    if (!pl || !pl->uploaded) return set_err(IMS_ERR_ARG, "plan is NULL or not uploaded");
    const int64_t n = pl->sizes.realized_count;
    if (n <= 0) return IMS_OK;
    if (!out_dev) return set_err(IMS_ERR_ARG, "out_dev is NULL");
    hipLaunchKernelGGL(k_scatter_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const int64_t*)(pl->arena_dev + pl->off_realized_where), (const double*)pl->realized_dev, out_dev, n);
    HIP_TRY(hipGetLastError());
    return IMS_OK;
}

}  // extern "C"
