// fleet_hostpath.hip -- the entries that take host pointers: fleet_reset_host, fleet_step_host and their _norm forms, what the
// last host step left behind (fleet_last_step_*), and pinned memory for callers.  Owns the copy workers and the order of a host
// step: actions up, the step (and the normaliser's launches), the small block and the observations down.
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>

#include "fleet_batch.h"
#include "fleet_norm.h"

namespace {

// Host-side copies of the host-pointer path (observations from the pinned landing buffer to a pageable destination): one core
// reads memory the device has just written at ~20 GB/s, so the pieces of a transfer are copied by a few worker threads while
// the calling thread waits for the next piece to land.  One pool per process, created at the first use and never torn down
// (its threads sleep on a condition variable); a forked child makes its own.
class CopyPool {
 public:
  static CopyPool* get() {
    static std::mutex mk;
    static CopyPool* pool = nullptr;
    std::lock_guard<std::mutex> g(mk);
    if (!pool || pool->pid_ != getpid()) pool = new CopyPool(3);  // (a fork leaves the parent's object behind: no threads in it)
    return pool;
  }
  void submit(void* dst, const void* src, size_t n) {
    pending_.fetch_add(1, std::memory_order_relaxed);
    {
      std::lock_guard<std::mutex> g(m_);
      q_.push_back({dst, src, n});
    }
    cv_.notify_one();
  }
  void wait() {  // all submitted copies done (the caller's own: calls on one handle are serialised, pools are per process)
    while (pending_.load(std::memory_order_acquire) != 0) std::this_thread::yield();
  }

 private:
  struct Task { void* dst; const void* src; size_t n; };
  explicit CopyPool(int workers) : pid_(getpid()) {
    for (int i = 0; i < workers; ++i) std::thread([this] { run(); }).detach();
  }
  void run() {
    for (;;) {
      Task t;
      {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [this] { return !q_.empty(); });
        t = q_.front();
        q_.pop_front();
      }
      memcpy(t.dst, t.src, t.n);
      pending_.fetch_sub(1, std::memory_order_release);
    }
  }
  pid_t pid_;
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<Task> q_;
  std::atomic<int> pending_{0};
};

}  // namespace

// fleet_step_host and fleet_step_host_norm: the step, then (with a normaliser) its three launches on the handle's stream, then
// the transfers -- the normalised observations from the normaliser's buffer, rewards normalised in place in the small block,
// terminal rows of done envs normalised in place before they are compacted
static int step_host_impl(fleet_handle h, fleet_norm_handle nrm, const void* actions, int act_dtype, float* obs, double* reward,
                          uint8_t* done, float* terminal_obs) {
  FLEET_ENTER(h);
  if (!h || !actions || !obs || !reward || !done || !act_dtype_ok(act_dtype)) {
    if (h) h->error = "fleet_step_host: null buffer or bad action dtype";
    return FLEET_ERR_INVALID;
  }
  if (nrm) {
    std::string why;
    if (fleet_norm_check_fit(nrm, h->d.E, h->d.obs_dim, h->device, &why) != FLEET_OK) {
      h->error = "fleet_step_host_norm: " + why;
      return FLEET_ERR_INVALID;
    }
  }
  HIP_TRY(h, hipSetDevice(h->device));
  const int E = h->d.E;
  const FleetSmallBlock& S = h->small;
  const size_t EN = (size_t)E * h->d.N;
  const size_t row = (size_t)h->d.obs_dim * sizeof(float);
  const size_t OD = (size_t)E * row;
  const size_t abytes = EN * (act_dtype == FLEET_ACT_F64 ? 8 : 4);
  // Action buffers from fleet_host_alloc are pinned: the transfer runs straight out of them.  Anything else goes through the
  // handle's pinned mirror (one small memcpy on the host instead of the runtime's pageable staging).
  hipPointerAttribute_t attr;
  auto pinned = [&](const void* p) {
    return hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeHost;
  };
  const bool act_pinned = pinned(actions);
  (void)hipGetLastError();  // hipPointerGetAttributes on a pageable pointer leaves an error code behind
  const void* asrc = actions;
  if (!act_pinned) {
    memcpy(h->pin_actions, actions, abytes);
    asrc = h->pin_actions;
  }
  HIP_TRY(h, hipMemcpyAsync(h->st_actions, asrc, abytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, fleet_launch_step(h->d, h->st_actions, act_dtype, 1, h->st_obs, h->st_reward, h->st_done,
                               terminal_obs ? h->st_term : nullptr, nullptr, h->stream));
  const float* obs_src = h->st_obs;
  if (nrm) {
    obs_src = fleet_norm_out_buffer(nrm);
    HIP_TRY(h, fleet_norm_enqueue_step(nrm, h->st_obs, h->st_reward, h->st_done, terminal_obs ? h->st_term : nullptr,
                                       fleet_norm_out_buffer(nrm), h->st_reward, terminal_obs ? h->st_term : nullptr, h->stream));
  }
  if (terminal_obs)
    HIP_TRY(h, fleet_launch_term_compact(h->d, h->st_done, h->st_term, S.idx(h->st_small), S.count(h->st_small), S.ep_return(h->st_small),
                                         S.ep_len(h->st_small), h->st_term_compact, h->stream));
  h->host_step_has_episodes = terminal_obs != nullptr;
  HIP_TRY(h, hipMemcpyAsync(h->pin_small, h->st_small, S.bytes, hipMemcpyDeviceToHost, h->stream));
  // The observations: straight into the caller's buffer at the link rate if it is pinned.  A pageable destination (a fresh
  // array per step, what the reference's env returns) gets them in pieces through a pinned landing buffer of the handle: each
  // piece is copied to its destination by this thread as soon as it has landed, while the following pieces are still on the
  // link -- the host copy (the slower of the two at 6 MB per step) hides the transfer instead of following it.
  const bool obs_pinned = pinned(obs);
  (void)hipGetLastError();
  if (obs_pinned || OD < (size_t)1 << 18) {
    HIP_TRY(h, hipMemcpyAsync(obs, obs_src, OD, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  } else {
    if (!h->pin_obs) {
      HIP_TRY(h, hipHostMalloc((void**)&h->pin_obs, OD, hipHostMallocDefault));
      for (auto& e : h->obs_piece_ev) HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // the first piece is small (the host copy starts early), the rest equal; boundaries on 4 KiB
    size_t cut[FleetEnvBatch::kObsPieces + 1];
    constexpr int P = FleetEnvBatch::kObsPieces;
    cut[0] = 0;
    const size_t first = (OD / (2 * (size_t)P)) & ~(size_t)4095;
    for (int c = 1; c < P; ++c) cut[c] = (first + (OD - first) * (size_t)(c - 1) / (size_t)(P - 1)) & ~(size_t)4095;
    cut[P] = OD;
    const char* src = reinterpret_cast<const char*>(obs_src);
    for (int c = 0; c < P; ++c) {
      if (cut[c + 1] > cut[c])
        HIP_TRY(h, hipMemcpyAsync(h->pin_obs + cut[c], src + cut[c], cut[c + 1] - cut[c], hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipEventRecord(h->obs_piece_ev[c], h->stream));
    }
    char* dst = reinterpret_cast<char*>(obs);
    CopyPool* pool = CopyPool::get();
    hipError_t werr = hipSuccess;
    constexpr int kSplit = 4;  // host copies per piece: three workers + (for the last piece) this thread
    for (int c = 0; c < P && werr == hipSuccess; ++c) {
      werr = hipEventSynchronize(h->obs_piece_ev[c]);
      if (werr != hipSuccess || cut[c + 1] <= cut[c]) continue;
      const size_t lo = cut[c], n = cut[c + 1] - cut[c];
      const bool last = (c + 1 == P);
      const int parts = last ? kSplit : kSplit - 1;
      for (int k = 0; k < parts; ++k) {
        const size_t a0 = lo + ((n * (size_t)k / parts) & ~(size_t)63);
        const size_t a1 = (k + 1 == parts) ? lo + n : lo + ((n * (size_t)(k + 1) / parts) & ~(size_t)63);
        if (last && k + 1 == parts) memcpy(dst + a0, h->pin_obs + a0, a1 - a0);  // nothing left to wait for: this thread copies too
        else pool->submit(dst + a0, h->pin_obs + a0, a1 - a0);
      }
    }
    pool->wait();
    HIP_TRY(h, werr);
  }
  memcpy(reward, S.reward(h->pin_small), (size_t)E * 8);
  memcpy(done, S.done(h->pin_small), (size_t)E);
  h->last_step_err = *S.err_word(h->pin_small);  // came with the rewards
  if (terminal_obs) {
    // terminal observations only exist for the envs that finished in this step: only those rows cross PCIe; rows of envs
    // that did not finish are left untouched
    const int n = *S.count(h->pin_small);
    if (n > 0) {
      const int32_t* idx = S.idx(h->pin_small);
      HIP_TRY(h, hipMemcpyAsync(h->pin_term, h->st_term_compact, (size_t)n * row, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      for (int k = 0; k < n; ++k) memcpy(terminal_obs + (size_t)idx[k] * h->d.obs_dim, h->pin_term + (size_t)k * h->d.obs_dim, row);
    }
  }
  // Device error bits raised by this step (or left by an earlier one: they are sticky) are reported by this very call, like the
  // reference raises inside step(); the outputs above are complete.  No extra launch or transfer on the clean path.
  if (h->last_step_err) {
    (void)fleet_check_errors(h);  // names the env in fleet_last_error
    return FLEET_ERR_STATE;
  }
  return FLEET_OK;
}

extern "C" {

int fleet_reset_host(fleet_handle h, const uint8_t* mask, float* obs) {
  FLEET_ENTER(h);
  if (!h || !obs) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t OD = (size_t)h->d.E * h->d.obs_dim * sizeof(float);
  if (mask) {
    HIP_TRY(h, hipMemcpyAsync(h->st_mask, mask, h->d.E, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->st_obs, obs, OD, hipMemcpyHostToDevice, h->stream));  // keep unmasked rows as they were
  }
  HIP_TRY(h, fleet_launch_reset(h->d, mask ? h->st_mask : nullptr, h->st_obs, h->stream));
  HIP_TRY(h, hipMemcpyAsync(obs, h->st_obs, OD, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return FLEET_OK;
}

int fleet_step_host(fleet_handle h, const void* actions, int act_dtype, float* obs, double* reward, uint8_t* done,
                    float* terminal_obs) {
  return step_host_impl(h, nullptr, actions, act_dtype, obs, reward, done, terminal_obs);
}

int fleet_step_host_norm(fleet_handle h, fleet_norm_handle n, const void* actions, int act_dtype, float* obs, double* reward,
                         uint8_t* done, float* terminal_obs) {
  if (!n) {
    if (h) h->error = "fleet_step_host_norm: null normaliser";
    return FLEET_ERR_INVALID;
  }
  return step_host_impl(h, n, actions, act_dtype, obs, reward, done, terminal_obs);
}

int fleet_reset_host_norm(fleet_handle h, fleet_norm_handle n, float* obs) {
  FLEET_ENTER(h);
  if (!h || !obs) return FLEET_ERR_INVALID;
  std::string why;
  if (fleet_norm_check_fit(n, h->d.E, h->d.obs_dim, h->device, &why) != FLEET_OK) {
    h->error = "fleet_reset_host_norm: " + why;
    return FLEET_ERR_INVALID;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t OD = (size_t)h->d.E * h->d.obs_dim * sizeof(float);
  HIP_TRY(h, fleet_launch_reset(h->d, nullptr, h->st_obs, h->stream));
  HIP_TRY(h, fleet_norm_enqueue_reset(n, h->st_obs, fleet_norm_out_buffer(n), h->stream));
  HIP_TRY(h, hipMemcpyAsync(obs, fleet_norm_out_buffer(n), OD, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return FLEET_OK;
}

int fleet_last_step_error_bits(fleet_handle h, uint32_t* bits) {
  FLEET_ENTER(h);
  if (!h || !bits) return FLEET_ERR_INVALID;
  *bits = h->last_step_err;
  return FLEET_OK;
}

int fleet_last_step_episodes(fleet_handle h, int32_t* n, const int32_t** env_idx, const double** ep_return, const int32_t** ep_len) {
  FLEET_ENTER(h);
  if (!h || !n) return FLEET_ERR_INVALID;
  if (!h->host_step_has_episodes) {
    h->error = "fleet_last_step_episodes: needs a preceding fleet_step_host with a terminal_obs buffer";
    return FLEET_ERR_INVALID;
  }
  *n = *h->small.count(h->pin_small);
  if (env_idx) *env_idx = h->small.idx(h->pin_small);
  if (ep_return) *ep_return = h->small.ep_return(h->pin_small);
  if (ep_len) *ep_len = h->small.ep_len(h->pin_small);
  return FLEET_OK;
}

int fleet_host_alloc(size_t bytes, void** out) {
  if (!out || bytes == 0) return FLEET_ERR_INVALID;
  *out = nullptr;
  return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? FLEET_OK : FLEET_ERR_HIP;
}

int fleet_host_free(void* p) {
  if (!p) return FLEET_OK;
  return hipHostFree(p) == hipSuccess ? FLEET_OK : FLEET_ERR_HIP;
}

}  // extern "C"
