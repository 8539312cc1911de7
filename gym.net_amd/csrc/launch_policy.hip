// launch_policy.hip — a handle's launch configuration (h->lcfg): the one it starts with (the rules are launch_policy.hpp, a pure function;
// here the facts are read off the handle), what gymnet_vecenv_set_launch_policy may put in its place, and the entry points that report
// it.  Host code only: no kernels.
#include <hip/hip_runtime.h>

#include <cstring>

#include "handle.hpp"

using namespace gymnet;

namespace {

// The step kernel a launch with configuration `c` runs: the launcher's own selection (step_kernels.hpp select_step), its name and shape.
StepForm next_step_kernel(const gymnet_vecenv *h, const LaunchCfg &c) {
    if (h->f64) return h->launch_f64->select_step(h->autoreset, h->extras, c, h->n);
    return h->launch_f32->select_step(h->autoreset, h->extras, c, h->n);
}

// Applies the fields of `p` that are not -1.  A value the handle cannot run — or that would not take effect for it (a multi-lane form
// on a batch that is not whole groups, a reset form the env has no use for) — is an error and nothing changes.
// gymnet_vecenv_kernel_name stays the authority on what the next launch runs.
int apply_policy(gymnet_vecenv *h, const gymnet_launch_policy &p) {
    LaunchCfg c = h->lcfg;
    int graph_mode = h->graph.mode;
    const bool acrobot = h->cfg.env_id == GYMNET_ENV_ACROBOT;
    const bool wide2 = acrobot || h->f64;            // the env's wide form is two lanes per thread (else four)
    auto bad = [&](const char *what, int v) -> int {
        return fail(h, GYMNET_ERR_INVALID_ARG, "launch policy: %s = %d is not available for this handle", what, v);
    };
    if (p.vec != -1) {
        const bool ok = p.vec == 1 || (p.vec == 4 && h->can_vec4 && !wide2) || (p.vec == 2 && h->can_vec2 && wide2);
        if (ok) c.vec = p.vec; else return bad("vec", p.vec);
    }
    if (p.block != -1) { if (p.block == 64 || p.block == 128 || p.block == 256) c.block = p.block; else return bad("block", p.block); }
    if (p.nt != -1) { if (p.nt == 0 || p.nt == 12 || p.nt == 15) c.nt = p.nt; else return bad("nt", p.nt); }
    if (p.sequential_lanes != -1) {
        if (p.sequential_lanes >= 1 && p.sequential_lanes <= (h->f64 ? 4 : 5) && (acrobot || h->f64 || p.sequential_lanes == 1)) c.items = p.sequential_lanes;
        else return bad("sequential_lanes", p.sequential_lanes);
    }
    if (p.reset_form != -1) {
        const bool has_form1 = h->desc->alias;       // the wave-compacted reset hands back the state only (CartPole, MountainCar[Continuous])
        if (p.reset_form == 0 || (p.reset_form == 1 && has_form1)) c.reset_form = p.reset_form; else return bad("reset_form", p.reset_form);
    }
    if (p.lds_pipe != -1) {
        if (p.lds_pipe == 0 || (p.lds_pipe == 1 && h->lds_ok)) c.lds_pipe = p.lds_pipe; else return bad("lds_pipe", p.lds_pipe);
    }
    if (p.occupancy_lds_bytes != -1) {
        if (p.occupancy_lds_bytes >= 0 && p.occupancy_lds_bytes <= 160 * 1024) c.lds_bytes = p.occupancy_lds_bytes;
        else return bad("occupancy_lds_bytes", p.occupancy_lds_bytes);
    }
    if (p.graph != -1) { if (p.graph == 0 || p.graph == 1) graph_mode = p.graph; else if (p.graph == -2) graph_mode = -1; else return bad("graph", p.graph); }
    if (p.sequential_lanes > 1) {
        // an explicitly requested multi-lane form must be the one the launcher resolves to: lean variant, the lane
        // width it is defined for, whole 2 * items * 256-lane groups for the pair form
        const int rseq = next_step_kernel(h, c).sequential;
        if (rseq != p.sequential_lanes)
            return fail(h, GYMNET_ERR_INVALID_ARG, "launch policy: sequential_lanes = %d would not take effect for this handle (vec %d, %s variant, "
                        "%lld lanes: the launcher resolves to %d)", p.sequential_lanes, c.vec, h->extras ? "bookkeeping" : "lean", (long long)h->n, rseq);
    }
    h->graph.mode = graph_mode;
    if (std::memcmp(&c, &h->lcfg, sizeof c) != 0) {
        h->lcfg = c;
        drop_graphs(h);          // captured launches froze the old configuration
    }
    return GYMNET_OK;
}

}  // namespace

namespace gymnet {

// gathers what launch_policy.hpp's default_policy reads, calls it, stores the result
void default_policy(gymnet_vecenv *h) {
    PolicyFacts f;
    f.env_id = h->cfg.env_id; f.alias = h->desc->alias; f.bytes_per_step = (int)bytes_per_step(h);
    f.f64 = h->f64; f.autoreset = h->autoreset; f.n = h->n; f.simds = h->simds;
    f.rows16 = aligned16(h->d_state) && aligned16(h->d_obs) && (h->sstride % 4 == 0) && (h->ostride % 4 == 0) &&
               (!h->d_obs_alt || aligned16(h->d_obs_alt));
    f.rows8 = aligned_to(h->d_state, 8) && aligned_to(h->d_obs, 8) && (h->sstride % 2 == 0) && (h->ostride % 2 == 0) &&
              (!h->d_obs_alt || aligned_to(h->d_obs_alt, 8));
    f.can2_f64 = aligned16(h->d_state) && (h->sstride % 2 == 0) && (!h->d_state_alt || aligned16(h->d_state_alt));
    const DefaultPolicy p = default_policy(f);
    h->lcfg = p.cfg; h->can_vec4 = p.can_vec4; h->can_vec2 = p.can_vec2; h->lds_ok = p.lds_ok;
}

}  // namespace gymnet

extern "C" {

int gymnet_vecenv_launch_policy(gymnet_vecenv *h, int32_t *vec, int32_t *block, int32_t *nt, int32_t *sequential_lanes) {
    return guarded([&]() -> int {
    if (!h) return fail(nullptr, GYMNET_ERR_INVALID_ARG, "null handle");
    if (vec) *vec = h->lcfg.vec;
    if (block) *block = h->lcfg.block;
    if (nt) *nt = h->lcfg.nt;
    if (sequential_lanes) {      // what the launcher resolves to (lanes, or lane pairs, a thread works through one after another)
        *sequential_lanes = next_step_kernel(h, h->lcfg).sequential;
    }
    return GYMNET_OK;
    });
}

int gymnet_vecenv_kernel_name(gymnet_vecenv *h, char *buf, int32_t capacity) {
    return guarded([&]() -> int {
    if (!h || !buf || capacity < 1) return fail(h, GYMNET_ERR_INVALID_ARG, "null handle / buffer");
    next_step_kernel(h, h->lcfg).name(buf, (size_t)capacity);
    return GYMNET_OK;
    });
}

int gymnet_vecenv_set_launch_policy(gymnet_vecenv *h, const gymnet_launch_policy *p) {
    return guarded([&]() -> int {
    ENTER(h);
    if (!p) return fail(h, GYMNET_ERR_INVALID_ARG, "policy is null");
    if (p->struct_size != sizeof(gymnet_launch_policy))
        return fail(h, GYMNET_ERR_INVALID_ARG, "policy.struct_size %u != %zu (ABI mismatch)", p->struct_size, sizeof(gymnet_launch_policy));
    HIP_TRY(h, hipStreamSynchronize(h->stream));     // no launch of the old configuration is still being captured / replayed
    return apply_policy(h, *p);
    });
}

int gymnet_vecenv_get_launch_policy(gymnet_vecenv *h, gymnet_launch_policy *out) {
    return guarded([&]() -> int {
    if (!h || !out) return fail(h, GYMNET_ERR_INVALID_ARG, "null argument");
    out->struct_size = sizeof *out;
    out->vec = h->lcfg.vec; out->block = h->lcfg.block; out->nt = h->lcfg.nt; out->sequential_lanes = h->lcfg.items;
    out->reset_form = h->lcfg.reset_form; out->lds_pipe = h->lcfg.lds_pipe; out->occupancy_lds_bytes = h->lcfg.lds_bytes;
    out->graph = h->graph.mode;
    return GYMNET_OK;
    });
}

}  // extern "C"
