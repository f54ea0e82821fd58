// The climb's population step (mg_search_climb): search.next_population followed by
// search.population_seeds, as one function that the device (k_climb_select, one wave) and the host
// (mg_climb_select_host, the CPU test's entry) both compile.  On the device the loops marked "lanes"
// are strided over the wave and the barriers are real; on the host one "lane" runs them all.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIP_DEVICE_COMPILE__)
#define MG_CLIMB_LANE ((uint32_t)threadIdx.x)
#define MG_CLIMB_LANES 64u
#define MG_CLIMB_SYNC() __syncthreads()
#else
#define MG_CLIMB_LANE 0u
#define MG_CLIMB_LANES 1u
#define MG_CLIMB_SYNC() ((void)0)
#endif

constexpr uint32_t kClimbSlots = 32;              // MG_SCORED_SLOTS: a round's winners
constexpr uint32_t kClimbCands = 2 * kClimbSlots;  // ... plus at most 32 previous members
constexpr unsigned long long kClimbIndexMask = (1ull << 48) - 1ull;

// Where seed row r of candidate c lies.  Candidate c < 32 is slot c's winner: its seed rows are
// watch rows of the model launch, gathered through the row map.  Candidate 32 + m is member m of
// the previous population: its rows are the previous seed set's, [n_rows][n_prev].
struct ClimbRows {
  const uint32_t* srows;      // [32][ww]
  const uint32_t* watch_row;  // [n_rows]
  const uint32_t* prev_rows;  // [n_rows][n_prev]
  uint32_t ww, n_prev;
  __host__ __device__ uint32_t at(uint32_t c, uint32_t r) const {
    return c < kClimbSlots ? srows[(size_t)c * ww + watch_row[r]] : prev_rows[(size_t)r * n_prev + (c - kClimbSlots)];
  }
};

// the step's working set: LDS on the device
struct ClimbWork {
  unsigned long long index[kClimbCands];
  uint32_t viol[kClimbCands], hash[kClimbCands], order[kClimbCands], valid[kClimbCands];
  uint32_t kept[kClimbSlots];  // candidate numbers of the new population, best first
  uint32_t n, n_kept;
};

// the population order: violations, then this round's winners before previous members, then index
__host__ __device__ inline bool climb_less(const ClimbWork& w, uint32_t a, uint32_t b) {
  if (w.viol[a] != w.viol[b]) return w.viol[a] < w.viol[b];
  if ((a >= kClimbSlots) != (b >= kClimbSlots)) return a < kClimbSlots;
  return w.index[a] < w.index[b];
}

// slots: this round's 32 slot words at slots[s * slot_stride] (viol << 48 | i - start, ~0 empty).
// Leaves the new population in w.kept[0 .. w.n_kept) (w.viol / w.index of those candidates) and
// writes its seed rows to new_rows[r * w.n_kept + m], which must not overlap R.prev_rows.
__host__ __device__ inline void mg_climb_select(const ClimbRows& R, const unsigned long long* slots,
                                                uint32_t slot_stride, unsigned long long start, const uint32_t* prev_viol,
                                                const unsigned long long* prev_index, uint32_t n_rows, uint32_t beam,
                                                ClimbWork& w, uint32_t* new_rows) {
  const uint32_t lane = MG_CLIMB_LANE;
  // lanes: the candidates and a hash of each one's rows (FNV-1a over the words)
  for (uint32_t c = lane; c < kClimbCands; c += MG_CLIMB_LANES) {
    bool ok;
    if (c < kClimbSlots) {
      const unsigned long long word = slots[(size_t)c * slot_stride];
      ok = word != ~0ull;
      w.viol[c] = (uint32_t)(word >> 48);
      w.index[c] = start + (word & kClimbIndexMask);
    } else {
      ok = c - kClimbSlots < R.n_prev;
      w.viol[c] = ok ? prev_viol[c - kClimbSlots] : 0u;
      w.index[c] = ok ? prev_index[c - kClimbSlots] : 0ull;
    }
    uint32_t h = 2166136261u;
    if (ok)
      for (uint32_t r = 0; r < n_rows; r++) h = (h ^ R.at(c, r)) * 16777619u;
    w.hash[c] = h;
    w.valid[c] = ok;
  }
  MG_CLIMB_SYNC();
  // lanes: a candidate's place is the number of candidates before it (no two compare equal: an
  // index occurs once among the winners and once among the members)
  for (uint32_t c = lane; c < kClimbCands; c += MG_CLIMB_LANES) {
    uint32_t before = 0, n = 0;
    for (uint32_t o = 0; o < kClimbCands; o++) {
      n += w.valid[o];
      before += w.valid[o] && o != c && climb_less(w, o, c);
    }
    if (w.valid[c]) w.order[before] = c;
    if (c == 0) w.n = n;
  }
  MG_CLIMB_SYNC();
  // the walk (every lane takes the same steps): keep a candidate whose rows differ from every one
  // kept so far.  Unequal hashes mean different rows; equal hashes are settled by comparing the rows.
  uint32_t n_kept = 0;
  for (uint32_t t = 0; t < w.n && n_kept < beam; t++) {
    const uint32_t c = w.order[t];
    bool dup = false;
#if defined(__HIP_DEVICE_COMPILE__)
    bool eq = false;  // lane q looks at kept entry q
    if (lane < n_kept) eq = w.hash[w.kept[lane]] == w.hash[c];
    unsigned long long same = __ballot(eq);
    while (same && !dup) {
      const uint32_t k = w.kept[__ffsll((long long)same) - 1];
      same &= same - 1ull;
      bool differ = false;
      for (uint32_t r = lane; r < n_rows; r += MG_CLIMB_LANES) differ |= R.at(k, r) != R.at(c, r);
      dup = !__any(differ);
    }
#else
    for (uint32_t q = 0; q < n_kept && !dup; q++) {
      if (w.hash[w.kept[q]] != w.hash[c]) continue;
      dup = true;
      for (uint32_t r = 0; r < n_rows && dup; r++) dup = R.at(w.kept[q], r) == R.at(c, r);
    }
#endif
    if (!dup) w.kept[n_kept++] = c;  // the same store from every lane
    MG_CLIMB_SYNC();
  }
  w.n_kept = n_kept;
  MG_CLIMB_SYNC();
  // lanes: the new seed set
  for (uint32_t q = lane; q < n_rows * n_kept; q += MG_CLIMB_LANES)
    new_rows[q] = R.at(w.kept[q % n_kept], q / n_kept);
}
