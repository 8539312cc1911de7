// step_graph.hip — the rollout of `steps` vector steps, one kernel launch each, and its graph replay (h->graph): while the host launch
// path is the bottleneck a captured hipGraph of one turn of the action ring is replayed instead.  Holds the cache of captured graphs,
// its eviction, and drop_graphs for everyone who changes what a captured launch froze.  Host code only: no kernels.
#include <hip/hip_runtime.h>

#include <vector>

#include "handle.hpp"

namespace gymnet {

struct GraphEntry {
    const void *actions;
    int64_t len, stride, ring;
    int parity, cparity, cur;
    hipGraph_t graph;
    hipGraphExec_t exec;
    uint64_t last_use;
};
constexpr size_t kMaxGraphs = 8;       // per handle; least-recently-used entry is destroyed beyond this
struct GraphCache {
    std::vector<GraphEntry> entries;
    uint64_t clock = 0;
};

static void destroy_graph(GraphEntry &g) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
    g.exec = nullptr; g.graph = nullptr;
}

void drop_graphs(gymnet_vecenv *h) {
    if (!h->graph.cache) return;
    for (auto &g : h->graph.cache->entries) destroy_graph(g);
    delete h->graph.cache;
    h->graph.cache = nullptr;
}

// `steps` vector steps, one kernel launch each (caller has ENTERed the handle)
int rollout_steps(gymnet_vecenv *h, const void *d_actions, int64_t steps, int64_t action_stride, int64_t ring, int graph_mode) {
    if (!d_actions) return fail(h, GYMNET_ERR_INVALID_ARG, "d_actions is null");
    if (steps < 0 || ring < 1 || action_stride < 0) return fail(h, GYMNET_ERR_INVALID_ARG, "bad steps/ring/action_stride");
    if (h->lcfg.vec > 1 && (!aligned_to(d_actions, 4 * h->lcfg.vec) || (action_stride % h->lcfg.vec) != 0))
        return fail(h, GYMNET_ERR_INVALID_ARG, "d_actions and action_stride must be %d-byte aligned", 4 * h->lcfg.vec);
    const char *base = static_cast<const char *>(d_actions);
    auto slice = [&](int64_t t) -> const void * { return base + (size_t)((t % ring) * action_stride) * 4; };
    if ((h->cfg.flags & GYMNET_FLAG_VALIDATE_ACTIONS) && !h->desc->box_action && steps > 0) {
        // Discrete.Contains over every slice the rollout will read, before any state changes (one readback)
        uint32_t bad = 0;
        ST_TRY(count_bad_actions(h, steps < ring ? steps : ring, slice, &bad));
        if (bad) return fail(h, GYMNET_ERR_INVALID_ACTION, "Action is outside of the configured action space. (%u lane-steps, Discrete(%d))", bad, h->desc->action_n);
    }

    // graph length: a multiple of `ring` (so every replay starts at slice 0) and even (so the double-buffered
    // device tick, done-count halves and observation buffers are the same at every replay)
    int64_t glen = (ring % 2 == 0) ? ring : 2 * ring;
    int64_t t = 0;
    // Graph replay only pays while the host launch path (~3.5 us per launch) is the bottleneck: measured on
    // MI355X, replay beats eager launches up to ~2^18 CartPole lanes (2.6 vs 5.7 us/step at 2^16), ties at 2^19
    // and loses at 2^20 (8.08 vs 7.85 us/step: a kernel node costs more than a back-to-back stream launch).
    const bool launch_bound = (size_t)h->n * bytes_per_step(h) < ((size_t)24 << 20);
    if (graph_mode < 0) graph_mode = h->graph.mode;          // gymnet_vecenv_set_launch_policy(.graph)
    const bool use_graph = graph_mode >= 0 ? graph_mode != 0 : launch_bound;
    if (use_graph && glen <= 4096 && steps >= glen) {
        const int parity = h->tslot, cparity = (int)(h->step_launches & 1u), cur = h->cur;
        if (!h->graph.cache) h->graph.cache = new GraphCache();
        std::vector<GraphEntry> &graphs = h->graph.cache->entries;
        GraphEntry *ge = nullptr;
        for (auto &g : graphs)
            if (g.actions == d_actions && g.len == glen && g.stride == action_stride && g.ring == ring && g.parity == parity &&
                g.cparity == cparity && g.cur == cur)
                ge = &g;
        if (!ge) {
            const uint64_t tick0 = h->tick, sl0 = h->step_launches, ls0 = h->lane_steps;
            const int slot0 = h->tslot, cur0 = h->cur, lcp0 = h->last_cparity;
            HIP_TRY(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
            int st = GYMNET_OK;
            for (int64_t k = 0; k < glen && st == GYMNET_OK; ++k) st = launch_one_step(h, slice(k));
            hipGraph_t graph = nullptr;
            hipError_t e = hipStreamEndCapture(h->stream, &graph);
            // capturing launched nothing: rewind the host mirrors (glen is even, so the buffer pair is back where it was)
            h->tick = tick0; h->step_launches = sl0; h->lane_steps = ls0; h->tslot = slot0; h->last_cparity = lcp0;
            if (h->cur != cur0) swap_buffers(h);
            if (st != GYMNET_OK) { if (graph) (void)hipGraphDestroy(graph); return st; }
            if (e != hipSuccess) return fail(h, GYMNET_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
            hipGraphExec_t exec = nullptr;
            e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            if (e != hipSuccess) { (void)hipGraphDestroy(graph); return fail(h, GYMNET_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e)); }
            if (graphs.size() >= kMaxGraphs) {   // a trainer that keeps reallocating its action buffer must not leak graphs
                size_t lru = 0;
                for (size_t i = 1; i < graphs.size(); ++i) if (graphs[i].last_use < graphs[lru].last_use) lru = i;
                HIP_TRY(h, hipStreamSynchronize(h->stream));          // the evicted exec may still be running
                destroy_graph(graphs[lru]);
                graphs.erase(graphs.begin() + (long)lru);
            }
            graphs.push_back(GraphEntry{d_actions, glen, action_stride, ring, parity, cparity, cur, graph, exec, 0});
            ge = &graphs.back();
        }
        ge->last_use = ++h->graph.cache->clock;
        for (; t + glen <= steps; t += glen) {
            HIP_TRY(h, hipGraphLaunch(ge->exec, h->stream));
            h->tick += (uint64_t)glen;
            h->step_launches += (uint64_t)glen;
            h->lane_steps += (uint64_t)glen * (uint64_t)h->n;
            h->last_cparity = (int)((h->step_launches - 1) & 1u);
        }
    }
    for (; t < steps; ++t) ST_TRY(launch_one_step(h, slice(t)));
    return GYMNET_OK;
}

}  // namespace gymnet
