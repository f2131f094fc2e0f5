// The one text of how device and pinned buffers are allocated, released and grown (host only: no kernel needs this).
//
// The state structs keep their raw pointers and capacities and their explicit *_free functions; nothing here owns
// anything.  A site says in one line which rule it uses:
//   device_alloc / pinned_alloc, device_release / pinned_release   typed hipMalloc / hipHostMalloc, "free and forget";
//                                  what a group site (one booking, one capacity, many buffers) is written with
//   slack_cap(need, slack)         the capacity a growth asks for
//   grow_device / grow_pinned      one buffer with its own capacity; the contents are discarded
//   grow_device_keep               ... the first `keep` elements move to the new buffer
//   grow_group_keep                the same for buffers that share one capacity, all or nothing
// `who` is the CALLER's __func__: a growth is booked on it (note_alloc).  A null `who` books nothing — the sites that never
// booked (DESIGN §3 lists them) stay unbooked.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "gpd_internal.h"

namespace gpd {

// elements of void are bytes
template <typename T>
constexpr size_t elem_bytes() {
  return sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
}

// `count` elements of T; the pointer is null on failure
template <typename T>
hipError_t device_alloc(T *&p, size_t count) {
  const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), count * elem_bytes<T>());
  if (e != hipSuccess) p = nullptr;
  return e;
}
template <typename T>
hipError_t pinned_alloc(T *&p, size_t count) {
  const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), count * elem_bytes<T>(), 0);
  if (e != hipSuccess) p = nullptr;
  return e;
}
// free and forget, in the order given: a null pointer is skipped, every pointer is null afterwards
template <typename... T>
void device_release(T *&...p) {
  ((p ? (void)hipFree(p) : (void)0), ...);
  ((p = nullptr), ...);
}
template <typename... T>
void pinned_release(T *&...p) {
  ((p ? (void)hipHostFree(p) : (void)0), ...);
  ((p = nullptr), ...);
}

// need + need / slack.  A rule with more to it is finished at its site from this one; an exact capacity is `need` itself.
template <typename N>
constexpr N slack_cap(N need, int slack) {
  return need + need / (N)slack;
}
static_assert(slack_cap(100, 4) == 125 && slack_cap(7, 4) == 8 && slack_cap(3, 4) == 3, "a quarter: most device buffers");
static_assert(slack_cap((size_t)100, 8) == 112 && slack_cap(100, 2) == 150, "an eighth (pinned records), a half");
static_assert(slack_cap(7, 4) + 1 == 7 + 1 + 7 / 4 && slack_cap(7 + 1, 4) == 10, "reserve_selection: k + 1 + k / 4, the slack of k and not of k + 1");
static_assert(slack_cap(4000, 4) + 1024 == 4000 + 4000 / 4 + 1024, "plane_reserve: a floor of slack on top");
static_assert(((slack_cap(1001, 4) + 3) & ~3) == 1252, "lenet_scratch_reserve: rounded up to whole groups of four images");
static_assert(slack_cap((size_t)10, 2) == 15 && slack_cap((size_t)1000, 2) == 1500, "SIS / label accumulators: max(.., 64), cut to the budget at the site");

// (keeps `need` and `grown` out of the deduction of N: an int need against a size_t capacity converts)
template <typename N>
using same_as = std::common_type_t<N>;

// One device buffer that only grows: `need` elements within its capacity cost nothing; beyond it the buffer is released and
// allocated again with `grown` elements, booked on `who`.  A failed allocation leaves it empty (null, capacity 0).
template <typename T, typename N>
int grow_device(T *&p, N &cap, same_as<N> need, same_as<N> grown, const char *who) {
  if (need <= cap) return GPD_OK;
  if (who) note_alloc(who);
  device_release(p);
  cap = 0;
  HIP_RET(device_alloc(p, (size_t)grown));
  cap = grown;
  return GPD_OK;
}
template <typename T, typename N>
int grow_pinned(T *&p, N &cap, same_as<N> need, same_as<N> grown, const char *who) {
  if (need <= cap) return GPD_OK;
  if (who) note_alloc(who);
  pinned_release(p);
  cap = 0;
  HIP_RET(pinned_alloc(p, (size_t)grown));
  cap = grown;
  return GPD_OK;
}

// A buffer of a group that shares one capacity: where its pointer lives, the bytes of one element, and whether its first
// elements move over when the group grows.
struct GroupBuffer {
  void **slot;
  size_t elem;
  bool kept;
};
template <typename T>
GroupBuffer group_buffer(T *&p, size_t elem, bool kept) {
  return {reinterpret_cast<void **>(&p), elem, kept};
}

// Moves a group to buffers of `cap` elements each: allocates all of them first, copies the first `keep` elements of the kept
// ones device to device on `stream` and waits for it, then releases the old buffers.  A failure of any allocation or of the copy
// releases what this call allocated and leaves the old buffers where they were.  The caller books and sets its capacity.
inline int grow_group_keep(std::initializer_list<GroupBuffer> group, size_t cap, size_t keep, hipStream_t stream) {
  constexpr size_t kMost = 4;
  char *fresh[kMost] = {nullptr, nullptr, nullptr, nullptr};
  hipError_t e = group.size() <= kMost ? hipSuccess : hipErrorInvalidValue;
  size_t i = 0;
  for (const GroupBuffer &b : group)
    if (e == hipSuccess) e = device_alloc(fresh[i++], cap * b.elem);
  i = 0;
  bool copied = false;
  for (const GroupBuffer &b : group) {
    if (e == hipSuccess && keep > 0 && b.kept && *b.slot) {
      e = hipMemcpyAsync(fresh[i], *b.slot, keep * b.elem, hipMemcpyDeviceToDevice, stream);
      copied = true;
    }
    i++;
  }
  if (e == hipSuccess && copied) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) {
    for (char *&q : fresh) device_release(q);
    set_error("moving buffers to a capacity of %zu elements failed: %s", cap, hipGetErrorString(e));
    return GPD_ERR_HIP;
  }
  i = 0;
  for (const GroupBuffer &b : group) {
    if (*b.slot) (void)hipFree(*b.slot);
    *b.slot = fresh[i++];
  }
  return GPD_OK;
}

// One device buffer that grows and keeps its first `keep` elements (grow_group_keep for a group of one, with its own
// capacity test and booking).
template <typename T>
int grow_device_keep(T *&p, size_t &cap, size_t need, size_t grown, size_t keep, hipStream_t stream, const char *who) {
  if (need <= cap) return GPD_OK;
  if (who) note_alloc(who);
  const int rc = grow_group_keep({group_buffer(p, elem_bytes<T>(), true)}, grown, keep, stream);
  if (rc == GPD_OK) cap = grown;
  return rc;
}

}  // namespace gpd
