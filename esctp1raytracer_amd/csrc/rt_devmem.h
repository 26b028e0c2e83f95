// rt_devmem.h -- who owns device memory.  The kernels' parameter blocks (rt_device.h SphGroups, TriGroups,
// TileLists, LightLists, LightBins) are plain structs of raw pointers passed by value, so the owner is a
// registry: it records which pointers it allocated and frees what is still recorded when it dies; the
// pointers themselves stay where they are.  No HIP header is needed here: the three device operations
// come from a backend (rt_capi.cpp over HIP, tests/devmem_main.cpp over malloc).
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "esctp1_rt.h"

namespace esc {

// ---- the backend; a failing call leaves its message with set_error
void *devmem_allocate(size_t bytes);      // nullptr when it fails
void devmem_free(void *p, size_t bytes);
bool devmem_wait(void *owner);            // until nothing the owner has queued still runs; false when it fails

class DevMem {
 public:
  // Call memory (epoch == nullptr): scratch and tables no recorded frame reads.
  // Frame memory: whatever a kernel launched by esc_render_strips reads or writes.  A recorded frame
  // (esc_frame) replays launches that hold these pointers, so FREEING one -- release, or the free half
  // of alloc / grow -- bumps *epoch and so ends every recorded frame; and while *capturing is set
  // (esc_frame_record's stream capture) nothing is touched and ESC_ERR_HIP comes back.  A first
  // allocation into a null pointer bumps nothing: a frame recorded before the buffer existed cannot
  // have used it.
  explicit DevMem(void *owner, uint64_t *epoch = nullptr, const bool *capturing = nullptr)
      : owner_(owner), epoch_(epoch), capturing_(capturing) {}
  DevMem(const DevMem &) = delete;
  DevMem &operator=(const DevMem &) = delete;
  ~DevMem() { release_all(); }

  // frees what p held, then allocates n elements; n == 0 leaves p null
  template <typename T> int alloc(T *&p, size_t n) {
    if (refuse()) return ESC_ERR_HIP;
    drop(p);
    p = nullptr;
    if (n == 0) return ESC_OK;
    p = static_cast<T *>(take(n * sizeof(T)));
    return p ? ESC_OK : ESC_ERR_HIP;
  }
  // grow-only scratch: nothing when cap >= need; else waits for the owner's stream (an earlier call may
  // still use the old buffer), frees, allocates `need` elements.  After a failed allocation p is null
  // and cap is 0, so the next call tries again.
  template <typename T> int grow(T *&p, size_t &cap, size_t need) {
    if (cap >= need) return ESC_OK;
    if (refuse() || !devmem_wait(owner_)) return ESC_ERR_HIP;
    cap = 0;
    const int rc = alloc(p, need);
    if (rc == ESC_OK) cap = need;
    return rc;
  }
  template <typename T> int release(T *&p) {
    if (refuse()) return ESC_ERR_HIP;
    drop(p);
    p = nullptr;
    return ESC_OK;
  }
  // the tables the kernels only read are `const T *` in the parameter blocks; the owner still owns them
  template <typename T> int alloc(const T *&p, size_t n) {
    T *q = const_cast<T *>(p);
    const int rc = alloc(q, n);
    p = q;
    return rc;
  }
  template <typename T> int release(const T *&p) {
    T *q = const_cast<T *>(p);
    const int rc = release(q);
    p = q;
    return rc;
  }
  void release_all() {
    if (epoch_ && !held_.empty()) ++*epoch_;
    for (const auto &h : held_) devmem_free(h.first, h.second);
    held_.clear();
  }
  // calls refused because a capture was open (esc_frame_record names the cause by it)
  unsigned refused() const { return refused_; }

 private:
  bool refuse() {
    if (!capturing_ || !*capturing_) return false;
    ++refused_;
    return true;
  }
  void drop(const void *p) {
    if (!p) return;
    for (auto &h : held_)
      if (h.first == p) {
        devmem_free(h.first, h.second);
        h = held_.back();
        held_.pop_back();
        if (epoch_) ++*epoch_;
        return;
      }
  }
  void *take(size_t bytes) {
    void *p = devmem_allocate(bytes);
    if (p) held_.emplace_back(p, bytes);
    return p;
  }
  void *owner_;
  uint64_t *epoch_;
  const bool *capturing_;
  unsigned refused_ = 0;
  std::vector<std::pair<void *, size_t>> held_;
};

} // namespace esc
