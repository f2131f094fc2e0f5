// The draw stream of Cloud::subsample (util/cloud.cpp:350-405).  The reference's generators are time-seeded, so the project's
// seeded stream is the definition: xorshift64 from 0x9E3779B97F4A7C15 ^ seed with the steps << 13, >> 7, << 17.  Plain C++ with
// no HIP in it: the host mirror (util::Cloud::subsample) and libgpd_hip.so (gpd_hip_sample_positions, the raw jobs of
// gpd_hip_detect_batch) draw from the same code.  Positions index a candidate list of n entries — the sample indices a cloud
// carries (drawn WITH repetition, as cloud.cpp:381-389) or the n points of the cloud itself (a partial Fisher-Yates, distinct).
#pragma once
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace gpd {
namespace sample {

struct Stream {
  uint64_t s;
  explicit Stream(uint32_t seed) : s(0x9E3779B97F4A7C15ull ^ (uint64_t)seed) {}
  uint64_t next() {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
  }
};

// num_draws positions into a list of n entries, each next() % n; num_draws >= n keeps the whole list in order
inline void with_repetition(int n, int num_draws, uint32_t seed, std::vector<int32_t> &out) {
  out.clear();
  if (n <= 0 || num_draws <= 0) return;
  if (num_draws >= n) {
    out.resize((size_t)n);
    for (int i = 0; i < n; i++) out[(size_t)i] = i;
    return;
  }
  Stream st(seed);
  out.resize((size_t)num_draws);
  for (int i = 0; i < num_draws; i++) out[(size_t)i] = (int32_t)(st.next() % (uint64_t)n);
}

// the first min(num_draws, n) entries of 0..n-1 after that many Fisher-Yates swaps (entry i with entry i + next() % (n - i)).
// The entries the swaps moved are kept in a map, so the cost is that of the draws, not of n.
inline void distinct(int n, int num_draws, uint32_t seed, std::vector<int32_t> &out) {
  out.clear();
  if (n <= 0 || num_draws <= 0) return;
  const int m = num_draws < n ? num_draws : n;
  Stream st(seed);
  std::unordered_map<int32_t, int32_t> moved;
  moved.reserve((size_t)m * 2);
  out.resize((size_t)m);
  for (int i = 0; i < m; i++) {
    const int j = i + (int)(st.next() % (uint64_t)(n - i));
    const auto at_j = moved.find(j);
    const int32_t vj = at_j == moved.end() ? j : at_j->second;
    const auto at_i = moved.find(i);
    const int32_t vi = at_i == moved.end() ? i : at_i->second;
    out[(size_t)i] = vj;  // entry i is final: later swaps touch positions > i only
    moved[j] = vi;
  }
}

}  // namespace sample
}  // namespace gpd
