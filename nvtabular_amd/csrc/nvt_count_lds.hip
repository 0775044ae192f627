// Path S of nvt_dense_count_* (paths 0 / 6 / 7): columns whose distinct keys fit workgroup-private
// LDS tables.  Two launches, no global hash table, no contended atomics; the design is described in
// front of lds_stage_kernel.  A table that fills up raises NVT_ST_OVERFLOW bit0 and the caller
// reruns the column on a larger path.
#include "nvt_common.hpp"
#include "nvt_internal.hpp"
#include "nvt_lds_table.hpp"

// key vectors per lane and batch of lds_stage_kernel.  4 was best while the misses of a batch were
// walked key position by key position; with every lane walking its own misses a batch costs as
// many probe chains as its unluckiest lane has misses, and 8 keys per lane beat 16 (p0 0.774 ->
// 0.738 ms, p6 0.505 -> 0.465 for the 13 LDS-resident Criteo columns; 1 vector: 0.765 / 0.464)
#ifndef NVT_STAGE_U
#define NVT_STAGE_U 2
#endif

namespace nvt {

// ---------------------------------------------------------------------------
// Path S.  Two launches, no tree:
//
//   stage 1  (256 << split_bits) workgroups.  Workgroup b owns row slab `slab` (grid-stride
//            over the column, 256 slabs) and key class q = low split_bits bits of slot_hash;
//            it counts the rows of its slab whose key is in its class into a private LDS
//            table.  With split_bits = 0 that is every row (<= ~11 k distinct keys); with
//            2 / 3 bits the column is read 4 / 8 times but tables hold a quarter / an
//            eighth of the vocabulary each (<= ~43 k / ~86 k distinct), which is still far
//            cheaper than one partition pass.  The 8 * SPLIT workgroups that share slabs
//            8g .. 8g+7 are consecutive block ids: block b runs on XCD b % 8, so all SPLIT
//            readers of a slab sit on ONE XCD and the re-reads are L2 hits.
//            The table is flushed GROUPED BY HOME RANGE (top 8 bits of the home slot) into
//            a fixed region per workgroup, with a 257-entry offset row -- no cursor atomics.
//   stage 2  one workgroup per (class q, range r): gathers segment r of the 256 partial
//            lists of class q (a wave per list) into a 512-slot LDS table and appends the
//            result to the output (one reservation atomic per workgroup).  Every key has
//            exactly one (q, r), so the merge is embarrassingly parallel: 1.9 M partial
//            entries (7 k-key column) merge in ~10 us instead of ~190 us for the former
//            32 -> 4 -> 1 workgroup tree.
// ---------------------------------------------------------------------------
constexpr int kSlabs = 256;     // row slabs of stage 1 (= workgroups per key class)
constexpr int kRanges = 256;    // home ranges per table
constexpr int kMergeBS = 256, kMergeSlots = 512;
constexpr unsigned kRepFill = 256;  // replicate hot keys per lane group while fill <= this

// hash of stage 1: home slot from bits >= kStageHomeShift, key class from the (up to 3) bits
// at kStageClassShift
__device__ __forceinline__ uint32_t stage_hash(int32_t key) { return mul24_hash(key); }
template <typename K>
struct StageBits {
  static constexpr int home = sizeof(K) == 4 ? 18 : 17, cls = sizeof(K) == 4 ? 15 : 0;
};
__device__ __forceinline__ uint64_t stage_hash(int64_t key) { return slot_hash(key); }
template <typename K, int SLOTS>
__device__ __forceinline__ uint32_t home_slot(K key) {
  return (uint32_t)(stage_hash(key) >> StageBits<K>::home) & (SLOTS - 1);
}
template <typename K>
__device__ __forceinline__ uint32_t key_class(K key, unsigned split_mask) {
  return (uint32_t)(stage_hash(key) >> StageBits<K>::cls) & split_mask;
}

template <typename K, typename C, int SLOTS>
__global__ __launch_bounds__(kStageBS) void lds_stage_kernel(
    const K *__restrict__ keys, const uint8_t *__restrict__ valid,
    const int64_t *__restrict__ weights, uint64_t n, int split_bits, int tiny, K *part_keys,
    int64_t *part_cnt, unsigned *seg_off, uint64_t *state) {
  constexpr K EMPTY = DKey<K>::empty;
  constexpr int VEC = DKey<K>::vec;
  __shared__ K lkeys[SLOTS];
  __shared__ C lcnt[SLOTS + kWave];  // + one scratch word per lane (see the unconditional add)
  __shared__ unsigned rcnt[kRanges], wtot[kRanges / kWave];
  __shared__ unsigned lfill, lovf, s_next;
  __shared__ unsigned long long s_nulls, s_sent;
  for (int i = threadIdx.x; i < SLOTS; i += kStageBS) {
    lkeys[i] = EMPTY;
    lcnt[i] = 0;
  }
  if (threadIdx.x < kRanges) rcnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    lfill = 0;
    lovf = 0;
    s_next = 0;
    s_nulls = 0;
    s_sent = 0;
  }
  __syncthreads();
  const unsigned split = 1u << split_bits, split_mask = split - 1;
  const unsigned q = (blockIdx.x >> 3) & split_mask;
  const unsigned slab = ((blockIdx.x >> (3 + split_bits)) << 3) | (blockIdx.x & 7);
  const unsigned nlists = gridDim.x;
  unsigned long long my_nulls = 0, my_sent = 0;
  bool failed = false;
  // A column with a handful of keys (Criteo has five with <= 14) makes every lane of a wave
  // hit the same 1-3 LDS words, and same-address LDS atomics serialise (106 us for 3 keys vs
  // 55 us for 36, tools/micro/lds_cfg_probe.hip).  On the `tiny` path (the caller expects
  // <= 64 distinct keys) each group of 8 lanes probes from its own offset: up to 8 copies
  // of a key, merged for free by stage 2 (duplicates within a partial list are legal).
  // A wrong expectation only costs duplicates: past kRepFill entries replication stops.
  // (Counting a sampled hot key in registers instead -- what P3 does for split buckets --
  // was tried here too: the extra compare per key costs more than the conflicts it removes,
  // +20 us per column; this loop is issue-bound, not LDS-bound.)
  uint32_t rep = tiny ? (lane_id() & 7u) * 2053u : 0u;
  auto add = [&](K key, unsigned long long w) {
    if (key == EMPTY) {
      if (q == 0) my_sent += w;
      return;
    }
    const auto h = stage_hash(key);
    if (((uint32_t)(h >> StageBits<K>::cls) & split_mask) != q) return;
    if (!lds_add<K, C, SLOTS>(lkeys, lcnt, &lfill, key, (C)w, (uint32_t)(h >> StageBits<K>::home) + rep))
      failed = true;
  };
  const uint64_t stride = (uint64_t)kSlabs * kStageBS;
  const uint64_t first = (uint64_t)slab * kStageBS + threadIdx.x;
  if (weights == nullptr) {
    const uint64_t nvec = n / VEC;
    using VecT = typename std::conditional<sizeof(K) == 4, int4, longlong2>::type;
    const VecT *vkeys = reinterpret_cast<const VecT *>(keys);
    // software pipeline: the U vectors of iteration i+1 are requested before iteration i is
    // pushed through the LDS table (one workgroup per CU: latency is covered by ILP, not TLP)
    constexpr int U = NVT_STAGE_U;
    VecT npack[U];
    unsigned nvb[U];
    // Each slab is a CONTIGUOUS range of the column, walked front to back in 16 KiB steps
    // (a grid-stride walk had every workgroup jump 4 MiB between consecutive loads: 1024
    // widely separated 16 KiB windows live at any time).
    const uint64_t per_slab = (nvec + kSlabs - 1) / kSlabs;
    const uint64_t slab_lo = (uint64_t)slab * per_slab;
    const uint64_t slab_hi = slab_lo + per_slab < nvec ? slab_lo + per_slab : nvec;
    // Round 6: a wave takes its batches of U x 64 consecutive vectors from a counter in LDS.  With a
    // fixed share per wave the oldest wave of a SIMD (it wins the issue arbitration) was through
    // with its share at 55 % of the loop's duration and the workgroup waited for the youngest one
    // with one wave per SIMD left to hide its LDS round trips (phase timers: 34-41 % of the kernel
    // between the first wave's last batch and the last wave's).
    constexpr uint64_t vstride = kWave;  // distance between the U vectors of one batch
    const uint64_t nbatch = (slab_hi > slab_lo ? slab_hi - slab_lo + vstride * U - 1 : 0) / (vstride * U);
    auto grab = [&]() -> uint64_t {
      unsigned c = 0;
      if (lane_id() == 0) c = atomicAdd(&s_next, 1u);
      return (uint64_t)__builtin_amdgcn_readfirstlane((int)c);
    };
    auto issue = [&](uint64_t v0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        uint64_t v = v0 + (uint64_t)u * vstride;
        nvb[u] = 0x10000;  // out of range
        if (v < slab_hi) {
          npack[u] = vkeys[v];
          nvb[u] = valid ? (unsigned)valid[(v * VEC) >> 3] : 0xFFu;  // raw byte, shifted later
        }
      }
    };
    uint64_t batch = grab();
    issue(slab_lo + batch * (vstride * U) + lane_id());
    unsigned fill_now = 0;  // refreshed with the batched home-slot reads below: a separate read
                            // here would drain every queued LDS atomic of the previous batch
    while (batch < nbatch) {
      const uint64_t v0 = slab_lo + batch * (vstride * U) + lane_id();
      if (fill_now > (unsigned)max_fill(SLOTS)) break;  // filling up: the column needs a larger path
      if (fill_now > kRepFill) rep = 0;
      VecT pack[U];
      unsigned vb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pack[u] = npack[u];
        vb[u] = nvb[u];
      }
      batch = grab();
      issue(slab_lo + batch * (vstride * U) + lane_id());   // (past the slab: no loads)
      // Probe in two sweeps.  Sweep 1 reads the HOME slot of every key of the batch -- U * VEC
      // independent LDS reads behind one wait; a key already sitting there (the common case
      // once the table is warm) only needs a fire-and-forget ds_add.  Sweep 2 walks the
      // probe chain for the rest.  One key at a time, each read -> compare -> add chain was
      // a full LDS round trip exposed to a workgroup with only 4 waves per SIMD: the loop
      // was latency-bound (which is also why masking 3/4 of the lanes never made it faster).
      constexpr int NKB = U * VEC;
      K kq[NKB];
      uint32_t hq[NKB];
      unsigned live = 0;  // bit q: key q is valid, of this class, not the sentinel
      // Branch-free classification (PMC: the per-key if / else ladders cost as many SALU
      // exec-mask instructions as there were VALU instructions, 37 + 36 per key).
      unsigned nnull = 0, nsent = 0;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool inrange = !(vb[u] & 0x10000);
        const unsigned bits =
            inrange ? (vb[u] >> (((v0 + (uint64_t)u * vstride) * VEC) & 7)) & ((1u << VEC) - 1u) : 0u;
        if constexpr (sizeof(K) == 4) {
          kq[u * VEC + 0] = pack[u].x;
          kq[u * VEC + 1] = pack[u].y;
          kq[u * VEC + 2] = pack[u].z;
          kq[u * VEC + 3] = pack[u].w;
        } else {
          kq[u * VEC + 0] = pack[u].x;
          kq[u * VEC + 1] = pack[u].y;
        }
        nnull += inrange ? (unsigned)VEC - (unsigned)__popc(bits) : 0u;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const int qi = u * VEC + j;
          const bool v = (bits >> j) & 1;
          const bool is_sent = v & (kq[qi] == EMPTY);
          const auto h = stage_hash(kq[qi]);
          const bool lv = v & !is_sent & (((uint32_t)(h >> StageBits<K>::cls) & split_mask) == q);
          nsent += is_sent ? 1u : 0u;
          hq[qi] = lv ? (((uint32_t)(h >> StageBits<K>::home) + rep) & (SLOTS - 1)) : 0u;
          live |= (lv ? 1u : 0u) << qi;
        }
      }
      my_nulls += nnull;
      if (q == 0) my_sent += nsent;
      K cur[NKB];
#pragma unroll
      for (int qi = 0; qi < NKB; ++qi) cur[qi] = lkeys[hq[qi]];
      fill_now = lfill;
      unsigned missbits = 0;
#pragma unroll
      for (int qi = 0; qi < NKB; ++qi) {
        const bool lv = (live >> qi) & 1;
        const bool hit = lv & (cur[qi] == kq[qi]);
        // unconditional add: lanes without a hit bump a per-lane scratch word past the table
        atomicAdd(&lcnt[hit ? hq[qi] : (uint32_t)SLOTS + lane_id()], (C)1);
        missbits |= ((lv & !hit) ? 1u : 0u) << qi;
      }
      // The probe chain of a miss is a loop of dependent LDS round trips, and with a few percent
      // of misses SOME lane misses at every one of the NKB key positions: walked position by
      // position the wave paid NKB chains per batch with a handful of lanes active in each.
      // Every lane walks ITS next miss instead: as many chains as the unluckiest lane has
      // misses (2-3 of 8 at a 7 % miss rate).
      while (__any(missbits != 0)) {
        if (missbits) {
          const int qm = (int)__ffs((int)missbits) - 1;
          K mk = kq[0];
          uint32_t mh = hq[0];
#pragma unroll
          for (int qi = 1; qi < NKB; ++qi) {
            mk = qm == qi ? kq[qi] : mk;
            mh = qm == qi ? hq[qi] : mh;
          }
          missbits &= missbits - 1u;
          if (!lds_add<K, C, SLOTS>(lkeys, lcnt, &lfill, mk, (C)1, mh)) failed = true;
        }
      }
    }
    for (uint64_t i = nvec * VEC + first; i < n; i += stride) {
      if (bit_valid(valid, i))
        add(keys[i], 1ull);
      else
        ++my_nulls;
    }
  } else {
    constexpr int UW = 4;
    for (uint64_t i0 = first; i0 < n; i0 += stride * UW) {
      const unsigned fill_now = lfill;
      if (fill_now > (unsigned)max_fill(SLOTS)) break;
      if (fill_now > kRepFill) rep = 0;
      K kk[UW];
      unsigned long long ww[UW];
      int st[UW];  // 0 = out of range, 1 = key, 2 = null row
#pragma unroll
      for (int u = 0; u < UW; ++u) {
        uint64_t i = i0 + (uint64_t)u * stride;
        st[u] = 0;
        if (i < n) {
          ww[u] = (unsigned long long)weights[i];
          st[u] = !bit_valid(valid, i) ? 2 : 1;
          if (st[u] == 1) kk[u] = keys[i];
        }
      }
#pragma unroll
      for (int u = 0; u < UW; ++u) {
        if (st[u] == 1)
          add(kk[u], ww[u]);
        else if (st[u] == 2)
          my_nulls += ww[u];
      }
    }
  }
  if (failed) atomicOr(&lovf, 1u);
  if (q == 0 && my_nulls) atomicAdd(&s_nulls, my_nulls);
  if (my_sent) atomicAdd(&s_sent, my_sent);
  __syncthreads();
  if (lovf || lfill > (unsigned)max_fill(SLOTS)) {
    if (threadIdx.x == 0) atomicOr((unsigned long long *)&state[DS_OVF], 1ull);
    // stage 2 must not read stale offsets from this list
    for (int r = threadIdx.x; r <= kRanges; r += kStageBS) seg_off[(uint64_t)r * nlists + blockIdx.x] = 0;
    return;
  }
  if (threadIdx.x == 0) {
    if (s_nulls) atomicAdd((unsigned long long *)&state[DS_NULLS], s_nulls);
    if (s_sent) atomicAdd((unsigned long long *)&state[DS_SENT], s_sent);
    if (blockIdx.x == 0) atomicAdd((unsigned long long *)&state[DS_ROWS], (unsigned long long)n);
  }
  // ---- flush grouped by home range: LDS histogram -> scan -> ranked scatter ----
  constexpr int RSHIFT = (SLOTS == 16384 ? 14 : SLOTS == 8192 ? 13 : 12) - 8;
  for (int i = threadIdx.x; i < SLOTS; i += kStageBS) {
    K k = lkeys[i];
    if (k != EMPTY) atomicAdd(&rcnt[home_slot<K, SLOTS>(k) >> RSHIFT], 1u);
  }
  __syncthreads();
  unsigned mine = 0, inc = 0;
  if (threadIdx.x < kRanges) {
    mine = rcnt[threadIdx.x];
    inc = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      unsigned o = __shfl_up(inc, off, 64);
      if (lane_id() >= (unsigned)off) inc += o;
    }
    if (lane_id() == 63) wtot[threadIdx.x / kWave] = inc;
  }
  __syncthreads();
  if (threadIdx.x < kRanges) {
    unsigned wbase = 0;
    for (unsigned i = 0; i < threadIdx.x / kWave; ++i) wbase += wtot[i];
    const unsigned startv = wbase + inc - mine;
    rcnt[threadIdx.x] = startv;  // becomes the range's write cursor
    seg_off[(uint64_t)threadIdx.x * nlists + blockIdx.x] = startv;
    if (threadIdx.x == kRanges - 1)
      seg_off[(uint64_t)kRanges * nlists + blockIdx.x] = startv + mine;
  }
  __syncthreads();
  K *ok = part_keys + (uint64_t)blockIdx.x * max_fill(SLOTS);
  int64_t *oc = part_cnt + (uint64_t)blockIdx.x * max_fill(SLOTS);
  for (int i = threadIdx.x; i < SLOTS; i += kStageBS) {
    K k = lkeys[i];
    if (k != EMPTY) {
      unsigned pos = atomicAdd(&rcnt[home_slot<K, SLOTS>(k) >> RSHIFT], 1u);
      ok[pos] = k;
      oc[pos] = (int64_t)lcnt[i];
    }
  }
}

// Path S, stage 2: workgroup (q, r) merges segment r of the kSlabs partial lists of class q.
template <typename K>
__global__ __launch_bounds__(kMergeBS) void range_merge_kernel(
    const K *__restrict__ part_keys, const int64_t *__restrict__ part_cnt,
    const unsigned *__restrict__ seg_off, int split_bits, uint64_t region, K *out_keys,
    int64_t *out_cnt, uint64_t out_cap, uint64_t *state) {
  constexpr K EMPTY = DKey<K>::empty;
  using C = unsigned long long;
  __shared__ K lkeys[kMergeSlots];
  __shared__ C lcnt[kMergeSlots];
  __shared__ unsigned lfill, lovf, wsum[kMergeBS / kWave];
  __shared__ unsigned long long base_s;
  __shared__ int s_skip;
  for (int i = threadIdx.x; i < kMergeSlots; i += kMergeBS) {
    lkeys[i] = EMPTY;
    lcnt[i] = 0;
  }
  if (threadIdx.x == 0) {
    lfill = 0;
    lovf = 0;
    // stage 1 already overflowed: the result is discarded anyway
    s_skip = (int)(__hip_atomic_load(&state[DS_OVF], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1);
  }
  __syncthreads();
  if (s_skip) return;  // workgroup-uniform (read once by thread 0)
  const unsigned r = blockIdx.x & (kRanges - 1), q = blockIdx.x >> 8;
  const unsigned nlists = (unsigned)kSlabs << split_bits;
  const unsigned lane = lane_id(), w = threadIdx.x / kWave;
  // thread t owns list t of this class: segment bounds -> LDS, exclusive scan of the lengths
  // gives a flat index space over all 256 segments, so the loads below are independent and
  // balanced (a wave-per-list loop here was a 64-deep chain of dependent global loads).
  static_assert(kMergeBS == kSlabs, "one thread per partial list");
  __shared__ unsigned seg_lo[kSlabs], seg_start[kSlabs + 1];
  {
    const unsigned li = threadIdx.x;
    const unsigned b1 = ((((li >> 3) << split_bits) | q) << 3) | (li & 7);
    const unsigned lo = seg_off[(uint64_t)r * nlists + b1];
    const unsigned hi = seg_off[(uint64_t)(r + 1) * nlists + b1];
    const unsigned len = hi - lo;
    unsigned inc = len;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      unsigned o = __shfl_up(inc, off, 64);
      if (lane >= (unsigned)off) inc += o;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned wbase = 0;
    for (unsigned i = 0; i < w; ++i) wbase += wsum[i];
    seg_lo[li] = lo;
    seg_start[li] = wbase + inc - len;
    if (li == kSlabs - 1) seg_start[kSlabs] = wbase + inc;
  }
  __syncthreads();
  const unsigned total_in = seg_start[kSlabs];
  bool failed = false;
  constexpr int UM = 4;
  for (unsigned j0 = threadIdx.x; j0 < total_in; j0 += kMergeBS * UM) {
    if (lfill > (unsigned)max_fill(kMergeSlots)) break;  // too many keys for path 0
    K kk[UM];
    int64_t cc[UM];
    bool ok[UM];
#pragma unroll
    for (int u = 0; u < UM; ++u) {
      const unsigned j = j0 + u * kMergeBS;
      ok[u] = j < total_in;
      if (ok[u]) {
        unsigned a = 0, bnd = kSlabs;  // largest li with seg_start[li] <= j
        while (bnd - a > 1) {
          const unsigned m = (a + bnd) >> 1;
          if (seg_start[m] <= j) a = m; else bnd = m;
        }
        const unsigned b1 = ((((a >> 3) << split_bits) | q) << 3) | (a & 7);
        const uint64_t idx = (uint64_t)b1 * region + seg_lo[a] + (j - seg_start[a]);
        kk[u] = part_keys[idx];
        cc[u] = part_cnt[idx];
      }
    }
#pragma unroll
    for (int u = 0; u < UM; ++u)
      if (ok[u] && !lds_add<K, C, kMergeSlots>(lkeys, lcnt, &lfill, kk[u], (C)cc[u],
                                               (uint32_t)(slot_hash(kk[u]) >> 4)))
        failed = true;
  }
  if (failed) atomicOr(&lovf, 1u);
  __syncthreads();
  if (lovf || lfill > (unsigned)max_fill(kMergeSlots)) {
    if (threadIdx.x == 0) atomicOr((unsigned long long *)&state[DS_OVF], 1ull);
    return;
  }
  // compact (2 slots per thread) and append with one reservation
  constexpr int PER = kMergeSlots / kMergeBS;
  unsigned mine = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) mine += (lkeys[threadIdx.x * PER + j] != EMPTY);
  unsigned inc = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    unsigned o = __shfl_up(inc, off, 64);
    if (lane >= (unsigned)off) inc += o;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  unsigned wbase = 0, total = 0;
  for (unsigned i = 0; i < kMergeBS / kWave; ++i) {
    if (i < w) wbase += wsum[i];
    total += wsum[i];
  }
  if (total == 0) return;
  if (threadIdx.x == 0)
    base_s = atomicAdd(reinterpret_cast<unsigned long long *>(&state[DS_OUT]),
                       (unsigned long long)total);
  __syncthreads();
  if (base_s + total > out_cap) {
    if (threadIdx.x == 0) atomicOr((unsigned long long *)&state[DS_OVF], 2ull);
    return;
  }
  uint64_t pos = base_s + wbase + inc - mine;
  unsigned long long mx = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    K k = lkeys[threadIdx.x * PER + j];
    if (k != EMPTY) {
      unsigned long long c = lcnt[threadIdx.x * PER + j];
      out_keys[pos] = k;
      out_cnt[pos] = (int64_t)c;
      mx = c > mx ? c : mx;
      ++pos;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    unsigned long long o = __shfl_down(mx, off, 64);
    mx = o > mx ? o : mx;
  }
  if (lane == 0 && mx > 0) {
    unsigned long long *gm = reinterpret_cast<unsigned long long *>(&state[NVT_ST_MAXCOUNT]);
    if (mx > __hip_atomic_load(gm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(gm, mx);
  }
}

// ---- host side ------------------------------------------------------------------------------------
// path -> stage-1 key-class bits (0 / 6: one key class, 7: two)
inline int split_bits_of(int kind) { return kind == 7 ? 1 : 0; }
inline int stage_slots(int key_bytes, bool weighted) {
  return (weighted || key_bytes == 8) ? kLdsSlots : kLdsSlotsBig;
}

// The workspace: the partial lists of stage 1.  One walk yields the size (base == nullptr) and
// the pointers.
struct LdsCountWs {
  char *p1_keys;
  int64_t *p1_cnt;
  unsigned *seg_off;
};
static uint64_t lds_count_ws_layout(int kind, int key_bytes, bool weighted, char *base,
                                    LdsCountWs *w) {
  uint64_t off = 0;
  auto take = [&](uint64_t bytes) {
    char *p = base ? base + off : nullptr;
    off += pad16(bytes);
    return p;
  };
  const uint64_t nlists = (uint64_t)kSlabs << split_bits_of(kind);
  const uint64_t cap = nlists * max_fill(stage_slots(key_bytes, weighted));
  w->p1_keys = take(cap * key_bytes);
  w->p1_cnt = (int64_t *)take(cap * 8);
  w->seg_off = (unsigned *)take((kRanges + 1) * nlists * 4);
  return off;
}
uint64_t lds_count_ws_bytes(int kind, int key_bytes, bool weighted) {
  LdsCountWs w;
  return lds_count_ws_layout(kind, key_bytes, weighted, nullptr, &w);
}

// the two launches for tables of SLOTS slots with counts of type C
template <typename K, typename C, int SLOTS>
static int stage_pair(const nvt_count_col &c, int kind, const LdsCountWs &w, hipStream_t s) {
  const int sbits = split_bits_of(kind);
  lds_stage_kernel<K, C, SLOTS><<<(unsigned)kSlabs << sbits, kStageBS, 0, s>>>(
      (const K *)c.keys, c.valid, c.weights, c.n, sbits, kind == 6, (K *)w.p1_keys, w.p1_cnt,
      w.seg_off, c.state);
  NVT_CHECK_LAUNCH();
  range_merge_kernel<K><<<(unsigned)kRanges << sbits, kMergeBS, 0, s>>>(
      (const K *)w.p1_keys, w.p1_cnt, w.seg_off, sbits, (uint64_t)max_fill(SLOTS), (K *)c.out_keys,
      c.out_counts, c.out_capacity, c.state);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

template <typename K>
int lds_count(const nvt_count_col &c, int kind, hipStream_t s) {
  LdsCountWs w;
  lds_count_ws_layout(kind, (int)sizeof(K), c.weights != nullptr, (char *)c.ws, &w);
  // unweighted: every partial sum is < 2^32 (n is), so u32 counts and (int32 keys)
  // 16384-slot tables; weighted merges need u64 counts and use 8192 slots
  if (c.weights) return stage_pair<K, unsigned long long, kLdsSlots>(c, kind, w, s);
  if constexpr (sizeof(K) == 4)
    return stage_pair<K, unsigned, kLdsSlotsBig>(c, kind, w, s);
  else
    return stage_pair<K, unsigned, kLdsSlots>(c, kind, w, s);
}
template int lds_count<int32_t>(const nvt_count_col &, int, hipStream_t);
template int lds_count<int64_t>(const nvt_count_col &, int, hipStream_t);

}  // namespace nvt
