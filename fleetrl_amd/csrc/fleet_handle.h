// fleet_handle.h -- the host scaffold the normaliser (fleet_norm.hip), the rollout buffer (fleet_rollout.hip) and the replay buffer
// (fleet_replay.hip) share: what such a handle holds, how it is opened and closed, how it changes streams, how its HIP errors and
// its device error word become messages, and how a buffer's arrays are laid out; and what every family's entries share: where a
// refusal's message goes.  Host code only; nothing here launches a kernel, and nothing here builds a string outside an error branch.  (The env's own handle, `fleet_handle`, is not one of these: fleet_batch.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/fleet_hip.h"

struct FleetHandleBase {
  int device = 0;
  hipStream_t stream = nullptr, own_stream = nullptr;  // where the *_dev calls launch; the handle's own (NULL until handle_open)
  std::string error;                                   // *_last_error(handle)
  char* block = nullptr;                               // the handle's one device allocation
  uint32_t* err = nullptr;                             // the error word in it, for the handles that have one
};

// a buffer: `block` holds the arrays of layout L, then the error word
template <typename Layout>
struct FleetBufferBase : FleetHandleBase {
  Layout L{};

  template <typename T>
  T* array(int which, int row = 0) const {
    return reinterpret_cast<T*>(block + L.offset[which] + (uint64_t)row * L.row_bytes[which]);
  }
};

#define FLEET_HANDLE_TRY(h, expr)                                         \
  do {                                                                    \
    hipError_t _e = (expr);                                               \
    if (_e != hipSuccess) {                                               \
      (h)->error = std::string(#expr) + ": " + hipGetErrorString(_e);     \
      return FLEET_ERR_HIP;                                               \
    }                                                                     \
  } while (0)

// a refusal without a handle: "<entry>: <why>" into the family's thread-local string (*_last_error(NULL)); returns rc
inline int handle_refuse(std::string& no_handle, const char* entry, const std::string& why, int rc) {
  no_handle = std::string(entry) + ": " + why;
  return rc;
}

// The opening of an entry that looks at its arguments before its handle: `why` is what the family's check_* function found ("" when
// the arguments pass).  FLEET_OK to go on.  Otherwise FLEET_ERR_INVALID, with "<entry>: <why>" -- "null handle" when the arguments
// pass -- in h->error, or in the family's thread-local string when there is no handle.  H: anything with an `error`.
template <typename H>
inline int handle_enter(const char* entry, const std::string& why, H* h, std::string& no_handle) {
  if (h && why.empty()) return FLEET_OK;
  (h ? h->error : no_handle) = std::string(entry) + ": " + (why.empty() ? "null handle" : why.c_str());
  return FLEET_ERR_INVALID;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// workgroups for `items` items at `per_block` each: at least one, at most `max_blocks` (the kernels stride over the rest)
inline unsigned grid_for(size_t items, size_t per_block, size_t max_blocks) {
  const size_t want = (items + per_block - 1) / per_block;
  return (unsigned)(want < 1 ? 1 : (want < max_blocks ? want : max_blocks));
}

// `count` arrays of `rows` rows of row[i] bytes each, every array at a multiple of `align`, then one aligned slot for the error word
inline void handle_layout(const uint64_t* row, int count, uint64_t rows, uint64_t align, uint64_t* offset, uint64_t* bytes,
                          uint64_t* row_bytes, uint64_t* error_offset, uint64_t* total_bytes) {
  uint64_t off = 0;
  for (int i = 0; i < count; ++i) {
    offset[i] = off;
    row_bytes[i] = row[i];
    bytes[i] = row[i] * rows;
    off = (off + bytes[i] + align - 1) / align * align;
  }
  *error_offset = off;
  *total_bytes = off + align;
}

// The device half of *_create, after the parameters were validated: `device` exists, the handle's own stream on it, `bytes` bytes
// of device memory (not initialised).  A status other than FLEET_OK comes with the reason in *why, "the <noun>'s" in it; the handle
// is then the caller's to destroy (handle_close takes it in any state).
inline int handle_open(FleetHandleBase* h, int device, size_t bytes, const char* noun, std::string* why) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    *why = "no HIP device";
    return FLEET_ERR_NODEVICE;
  }
  if (device < 0 || device >= ndev) {
    *why = "device index out of range";
    return FLEET_ERR_INVALID;
  }
  h->device = device;
  if (hipSetDevice(device) != hipSuccess) {
    *why = "hipSetDevice failed";
    return FLEET_ERR_HIP;
  }
  if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
    *why = "hipStreamCreate failed";
    return FLEET_ERR_HIP;
  }
  h->stream = h->own_stream;
  void* q = nullptr;
  if (hipMalloc(&q, bytes) != hipSuccess) {
    (void)hipGetLastError();  // (the failure is reported here: it must not surface again from the caller's next HIP call)
    *why = std::string("hipMalloc of the ") + noun + "'s " + std::to_string(bytes) + " bytes failed";
    return FLEET_ERR_HIP;
  }
  h->block = static_cast<char*>(q);
  return FLEET_OK;
}

// handle_open for a buffer: the block of its layout, cleared (the host waits for that), and the error word in it
template <typename Layout>
inline int handle_open_buffer(FleetBufferBase<Layout>* b, int device, const char* noun, std::string* why) {
  const int rc = handle_open(b, device, b->L.total_bytes, noun, why);
  if (rc != FLEET_OK) return rc;
  b->err = reinterpret_cast<uint32_t*>(b->block + b->L.error_offset);
  if (hipMemset(b->block, 0, b->L.total_bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    *why = std::string("clearing the ") + noun + " failed";
    return FLEET_ERR_HIP;
  }
  return FLEET_OK;
}

// waits for the handle's streams, then frees the block and the stream of its own; a handle that was never opened has neither
inline void handle_close(FleetHandleBase* h) {
  if (!h->own_stream) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  (void)hipStreamSynchronize(h->own_stream);
  if (h->block) (void)hipFree(h->block);
  (void)hipStreamDestroy(h->own_stream);
}

// (the two functions below name their handle `r` because FLEET_HANDLE_TRY puts the expression's text into the message)

// the buffers' *_set_stream: what was enqueued on the old stream is waited for first
inline int handle_set_stream(FleetHandleBase* r, void* hip_stream) {
  FLEET_HANDLE_TRY(r, hipSetDevice(r->device));
  FLEET_HANDLE_TRY(r, hipStreamSynchronize(r->stream));
  r->stream = static_cast<hipStream_t>(hip_stream);  // (NULL is the null stream: torch's default stream has that handle)
  return FLEET_OK;
}

// the buffers' *_check_errors: reads the error word behind everything enqueued; when it is set, clears it and reports `message`
inline int handle_check_errors(FleetHandleBase* r, const char* message) {
  FLEET_HANDLE_TRY(r, hipSetDevice(r->device));
  uint32_t word = 0;
  FLEET_HANDLE_TRY(r, hipMemcpyAsync(&word, r->err, sizeof word, hipMemcpyDeviceToHost, r->stream));
  FLEET_HANDLE_TRY(r, hipStreamSynchronize(r->stream));
  if (!word) return FLEET_OK;
  FLEET_HANDLE_TRY(r, hipMemsetAsync(r->err, 0, sizeof word, r->stream));
  r->error = message;
  return FLEET_ERR_STATE;
}
