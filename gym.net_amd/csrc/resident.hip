// resident.hip — the host side of the resident kernel (GYMNET_FLAG_RESIDENT, kernels.hpp Mailbox; h->res): the mailbox's allocation and
// release, starting the kernel and telling it to leave, and one command through the mailbox.  This code spins on memory a GPU kernel
// writes: the order of the stores to exited / done_seq / cmd_seq is the protocol.  Host code only: no kernels.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>

#include "handle.hpp"

using namespace gymnet;

namespace {

// ~1.5 us per poll over PCIe: the resident kernel leaves after ~4-5 ms without a command (rounds 4-5: 40000 polls = 50-75 ms).  While
// it spins it occupies the handle's stream and one wave, and anything that waits for the WHOLE device — hipDeviceSynchronize,
// torch.cuda.synchronize(), a hipFree out of a caching allocator — or that serialises dispatch (rocprofv3 --pmc, AMD_SERIALIZE_KERNEL)
// waits for this timeout: it bounds what a host that mixes an env loop with other GPU work in one process can lose per
// such call.  A loop that steps back to back never sees it; a step after a longer pause pays one relaunch (~20 us, the launch path's
// cost).  GYMNET_FLAG_RESIDENT is opt-in in every facade for the same reason.
constexpr uint64_t kResidentIdlePolls = 3000;

// a polite busy-wait: the host thread spins on a cache line the GPU writes over PCIe
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#endif
}

template <class R>
int resident_start_typed(gymnet_vecenv *h) {
    StepArgsT<R> a = make_step_args<R>(h, h->res.mb_dev->actions);       // the kernel reads its actions straight from the mailbox
    ResetArgsT<R> r = make_reset_args<R>(h, nullptr);
    HIP_TRY(h, launchers<R>(h).resident(h->autoreset, h->extras, a, r, h->res.mb_dev, kResidentIdlePolls, h->stream));
    return GYMNET_OK;
}

int resident_start(gymnet_vecenv *h) {
    // the kernel picks the sequence number it continues from out of the mailbox: nothing is pending at this point
    __atomic_store_n(&h->res.mb->exited, 0u, __ATOMIC_RELAXED);
    __atomic_store_n(&h->res.mb->done_seq, h->res.seq, __ATOMIC_RELAXED);
    __atomic_store_n(&h->res.mb->cmd_seq, h->res.seq, __ATOMIC_RELEASE);
    ST_TRY(h->f64 ? resident_start_typed<double>(h) : resident_start_typed<float>(h));
    h->res.running = true;
    return GYMNET_OK;
}

// the kernel is gone (the stream has drained, or shows empty): the engine tick it kept in a register comes back through the mailbox
void resident_gone(gymnet_vecenv *h) {
    h->res.running = false;
    h->tick = h->res.mb->tick;
}

}  // namespace

namespace gymnet {

int resident_create(gymnet_vecenv *h) {
    void *blk = nullptr;
    hipError_t e = hipHostMalloc(&blk, kMailboxBytes, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return fail(nullptr, GYMNET_ERR_HIP, "hipHostMalloc(&blk, kMailboxBytes, hipHostMallocMapped | hipHostMallocCoherent) failed: %s", hipGetErrorString(e));
    std::memset(blk, 0, kMailboxBytes);
    h->res.mb = static_cast<Mailbox *>(blk);
    void *dev = nullptr;
    e = hipHostGetDevicePointer(&dev, blk, 0);
    if (e != hipSuccess) return fail(nullptr, GYMNET_ERR_HIP, "hipHostGetDevicePointer(&dev, blk, 0) failed: %s", hipGetErrorString(e));
    h->res.mb_dev = static_cast<Mailbox *>(dev);
    h->res.enabled = true;
    return GYMNET_OK;
}

// (resident_stop has drained the stream, so nothing reads the mailbox any more)
void resident_release(gymnet_vecenv *h) {
    if (h->res.running) (void)resident_stop(h);
    if (h->res.mb) (void)hipHostFree(h->res.mb);
    h->res = Resident{};
}

// Tells a running resident kernel to leave and waits until it has; the engine tick it kept in a register comes back through
// the mailbox (and through both halves of d_tick2 for the next launch).
int resident_stop(gymnet_vecenv *h) {
    if (!h->res.running) return GYMNET_OK;
    if (!__atomic_load_n(&h->res.mb->exited, __ATOMIC_ACQUIRE)) {
        h->res.mb->cmd = kMailboxExit;
        __atomic_store_n(&h->res.mb->cmd_seq, ++h->res.seq, __ATOMIC_RELEASE);
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    resident_gone(h);
    return GYMNET_OK;
}

// One command through the mailbox: post it, wait for its results, copy them out.  actions: host, or NULL (resets).
int resident_command(gymnet_vecenv *h, uint32_t cmd, const void *actions, void *obs_out, float *reward_out, uint8_t *done_out) {
    const EnvDesc &d = *h->desc;
    if (h->res.running && __atomic_load_n(&h->res.mb->exited, __ATOMIC_ACQUIRE)) ST_TRY(resident_stop(h));   // it timed out since the last call
    if (!h->res.running) ST_TRY(resident_start(h));
    if (actions) std::memcpy(h->res.mb->actions, actions, (size_t)h->n * 4);
    h->res.mb->cmd = cmd;
    const uint64_t seq = ++h->res.seq;
    __atomic_store_n(&h->res.mb->cmd_seq, seq, __ATOMIC_RELEASE);
    uint64_t spins = 0;
    const auto t_start = std::chrono::steady_clock::now();
    while (__atomic_load_n(&h->res.mb->done_seq, __ATOMIC_ACQUIRE) != seq) {
        if ((++spins & 0x3FFu) == 0) {
            if (__atomic_load_n(&h->res.mb->exited, __ATOMIC_ACQUIRE)) {
                // the kernel left (idle timeout) in the instant this command was posted, without serving it: it touches
                // nothing any more — wait for it to be gone, start a new one, which finds the command pending
                HIP_TRY(h, hipStreamSynchronize(h->stream));
                resident_gone(h);
                if (__atomic_load_n(&h->res.mb->done_seq, __ATOMIC_ACQUIRE) == seq) break;
                __atomic_store_n(&h->res.mb->exited, 0u, __ATOMIC_RELAXED);
                ST_TRY(h->f64 ? resident_start_typed<double>(h) : resident_start_typed<float>(h));
                h->res.running = true;
            } else if (hipStreamQuery(h->stream) == hipSuccess) {
                // the stream is empty although nobody answered: the kernel is gone.  Nothing will ever read the posted command; resync
                // the tick from what the kernel last published so that the next call starts a fresh kernel on consistent state
                resident_gone(h);
                __atomic_store_n(&h->res.mb->done_seq, seq, __ATOMIC_RELAXED);      // the command is void: a restarted kernel must not run it late
                return fail(h, GYMNET_ERR_HIP, "the resident kernel ended without answering command %llu", (unsigned long long)seq);
            }
            if (std::chrono::steady_clock::now() - t_start > std::chrono::seconds(10)) {
                //  do not leave the command in the mailbox for a late-waking kernel to apply to NEWER actions: overwrite it
                // with EXIT, wait until the kernel has left (it publishes its tick on the way out), void the sequence number
                h->res.mb->cmd = kMailboxExit;
                __atomic_store_n(&h->res.mb->cmd_seq, ++h->res.seq, __ATOMIC_RELEASE);
                (void)hipStreamSynchronize(h->stream);
                resident_gone(h);
                return fail(h, GYMNET_ERR_HIP, "the resident kernel did not answer command %llu within 10 s; it has been stopped and the next call starts a new one",
                            (unsigned long long)seq);
            }
        }
        cpu_relax();
    }
    const char *mb_obs = reinterpret_cast<const char *>(h->res.mb) + kMailboxObsOffset;
    if (obs_out) std::memcpy(obs_out, mb_obs, (size_t)h->n * d.obs_dim * h->esz);
    if (reward_out) std::memcpy(reward_out, h->res.mb->reward, (size_t)h->n * 4);
    if (done_out) std::memcpy(done_out, h->res.mb->done, (size_t)h->n);
    h->tick = h->res.mb->tick;
    if (cmd == kMailboxStep) h->lane_steps += (uint64_t)h->n;
    else touch_epoch(h);      // a reset the resident kernel served: new observations outside a step launch
    return GYMNET_OK;
}

// the resident path serves this handle's host-boundary steps right now (everything that changes what the kernel's arguments
// describe — seeds, per-lane keys, state, policy — goes through ENTER, which makes the kernel leave first; it restarts with fresh arguments)
bool resident_serves(const gymnet_vecenv *h) { return h->res.enabled && !h->async_pending; }

}  // namespace gymnet
