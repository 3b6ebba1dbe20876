// Full-vocabulary sampler: top_k = 0 or > 64, with or without top_p (README "Full-vocabulary sampling";
// ops/reference.py::nucleus_sample is the definition). One launch, no host sync, hipGraph-capturable.
//
// The survivors of top-k / top-p are a prefix of the row in (logit descending, index ascending) order, so they are
// {key > T} plus the n_eq lowest-index tokens with key == T. The kernel finds (T, n_eq) by radix descent and then takes
// one Gumbel-max over the survivors, with noise keyed by the token's vocabulary index: nothing is sorted, and no
// candidate list leaves the chip.
//
// Split: one 512-thread workgroup per row, streaming the row with 16-byte loads (0.5 MB at V = 128256: the first
// sweep brings it into L2, the later ones re-read it there).
//   sweep 1      row maximum (as a key) -> m = max l. top_k = 0 with top_p >= 1 goes straight to the draw.
//   descent      32 key bits in three passes of 11 / 11 / 10 bits. Each pass fills two LDS histograms over the keys
//                that match the prefix found so far: count (u32) and mass (u64). A token's mass is the integer
//                uint64(exp2((l - m) * log2e) * 2^40), added with LDS integer atomics: integer addition is
//                order-independent, so every call writes the same bits. V <= 2^22 keeps the sums below 2^63. One wave
//                scans the bins from the top; the boundary bin is the first at which the cumulative count reaches k
//                (count descent) or the cumulative mass reaches ceil(top_p * Z) (mass descent; the product in fp64).
//                With both cuts the count descent runs first and yields Z = the mass of the top k; the mass cut is
//                then never looser than the count cut (rank k has exactly Z before it, and ceil(top_p * Z) <= Z), so
//                the mass descent's (T, n_eq) is the tighter of the two. At the last level all keys of the boundary
//                bin are equal and so are their masses mu: n_eq = ceil(remaining target / mu).
//   compaction   if the first pass's boundary bin holds at most NS_CAP keys they are written to an LDS list in index
//                order (a block scan per tile assigns the slots) and passes 2 and 3 run from LDS; a fuller bin (flat
//                or clustered rows) streams the row again.
//   tie index    if only some of the keys == T survive, the index of the n_eq-th of them is found once (from the list,
//                or by one more ordered sweep with a block scan per tile), so the draw needs no scan of its own.
//   draw         each thread walks its float4 groups in index order; one Philox4x32-10 call covers the four indices of
//                a group (counter = (i >> 2, row, step, 1): word 3 = 1 keeps the stream apart from topk_sample's).
//                score = l + gumbel; thread best -> wave reduce -> LDS reduce, ties to the lower index.
//
// min_p and typical_p (template parameters MINP / TYP; with both off the kernel is the one above):
//   min_p        token i passes iff mass_i >= min_mass = ceil(min_p * 2^40) (the product in fp64, on the host). The
//                mass is monotone in the key, so the cut is a second lower bound on the key: kmin = the smallest key
//                whose mass reaches min_mass, found once per row by bisection over the key bits (<= 32 evaluations).
//                Alone it needs no descent: max sweep, then the draw. Call the survivors so far S2.
//   typical      one sweep over S2 adds Z2 = sum mass_i and W = sum uint64(fp64(mass_i) * fp64(t_i)), t_i = m - l_i in
//                fp32 (thread sums -> wave reduce -> LDS integer atomics: the same bits every call). With p_i =
//                mass_i / Z2, -log p_i - H = t_i - h where h = W / Z2 (the log Z2 terms cancel), so the distance is
//                d_i = |t_i - h| with h = fp32(fp64(W) / fp64(Z2)). d_i >= 0, so its bits are monotone, and ~bits(d_i)
//                is a key whose descending order is d ascending: the same mass descent as top-p runs on that key over
//                S2 only, with target ceil(typical_p * Z2), and the bins scanned "from the top" are the smallest
//                distances. Its compaction reuses the LDS list (which then keeps the logit, from which key and mass
//                follow); the first descent's tie index is settled before. Keys that tie in d need not have equal
//                masses (one token above h and one below it), so the cut inside the tie group is an ordered mass scan:
//                the index at which the group's cumulative mass, in index order, reaches the remaining target.
//   kept         with either option the draw sweep counts the survivors it scores.
//
// LDS: 512 threads so that two workgroups share a CU; 2048 x (8 + 4) B of histograms + NS_CAP = 4096 x 8 B of list =
// 56 KB, under the 64 KB a workgroup may declare statically and two of them under the CU's 160 KB.
//
// -inf logits (the processors' bans) have mass 0 and score -inf: never drawn while the row has a finite logit. A row
// that is all -inf is sampled as a row of equal logits.
#include "common.h"
#include "launchers.h"
#include "sampler_keys.h"

namespace jla {

namespace {

constexpr int NS_THREADS = 512, NS_WAVES = NS_THREADS / 64, NS_BINS = 2048, NS_CAP = 4096;
constexpr int NS_MAX_V = 1 << 22;
typedef unsigned long long u64_t;

struct NsShared {
  u64_t mass[NS_BINS];
  uint32_t cnt[NS_BINS];
  uint32_t lkey[NS_CAP];  // compacted boundary bin: keys and vocabulary indices, in index order
  int32_t lidx[NS_CAP];
  uint32_t wsum[NS_WAVES];
  u64_t wsum64[NS_WAVES];
  u64_t z2, w;                           // typical: the mass of S2 and its mass-weighted sum of m - l
  u64_t sel_above_m, sel_bin_m, sel_tr;  // written by the scanning wave
  uint32_t sel_bin, sel_above_c, sel_bin_c;
  float red_s[NS_WAVES];
  int32_t red_i[NS_WAVES];
  uint32_t red_k[NS_WAVES], red_c[NS_WAVES];
  int32_t tie_idx;
};

struct NsRow {
  const float* x;
  int V, n4;  // n4 = groups of four consecutive indices
  bool vec;   // 16-byte loads (V % 4 == 0, V >= 1024, aligned base); otherwise the scalar tail path
  bool dead;  // every logit is -inf: sampled as equal logits
  float inv_t, m;
};

// the logits of group i4 (indices 4 * i4 ..); returns how many of them are inside the row
JLA_DEV int ns_load4(const NsRow& r, int i4, float (&v)[4]) {
  if (r.vec) {
    const float4 t = reinterpret_cast<const float4*>(r.x)[i4];
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    return 4;
  }
  const int n = min(4, r.V - 4 * i4);
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = q < n ? r.x[4 * i4 + q] : 0.f;
  return n;
}

// l = x * inv_t, one rounded multiply (never contracted into the subtraction or addition that follows)
JLA_DEV float ns_l(const NsRow& r, float x) { return r.dead ? 0.f : __fmul_rn(x, r.inv_t); }

JLA_DEV u64_t ns_mass(const NsRow& r, float x) {
  return (u64_t)(exp2f(__fsub_rn(ns_l(r, x), r.m) * 1.4426950408889634f) * 1099511627776.0f);
}

// exclusive block scan of one value per thread (uint32 counts; uint64 masses); total = the block's sum
template <typename T>
JLA_DEV T ns_block_scan_in(T v, T* wsum, T& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NS_WAVES; ++i) {
    if (i < w) base += wsum[i];
    tot += wsum[i];
  }
  __syncthreads();
  total = tot;
  return base + incl - v;
}
JLA_DEV uint32_t ns_block_scan(uint32_t v, NsShared& sh, uint32_t& total) {
  return ns_block_scan_in(v, sh.wsum, total);
}
JLA_DEV u64_t ns_block_scan(u64_t v, NsShared& sh, u64_t& total) { return ns_block_scan_in(v, sh.wsum64, total); }

// The survivors of top-k / top-p (S1: key > T, and key == T up to index tie_idx) and of min_p (key >= kmin).
struct NsKeep {
  bool all;  // no top-k and no top-p cut
  uint32_t T, kmin;
  int32_t tie_idx;
  JLA_DEV bool operator()(uint32_t key, int i) const {
    return (all || key > T || (key == T && i <= tie_idx)) && key >= kmin;
  }
};

// What a descent orders by. in(): whether token i takes part; key(): a larger key comes earlier; pack() / unpack():
// the word the compacted list keeps of a token, and the key and logit it gives back.
struct NsLogitKey {
  JLA_DEV bool in(int, float) const { return true; }
  JLA_DEV uint32_t key(float x) const { return fkey(x); }
  JLA_DEV uint32_t pack(float, uint32_t key) const { return key; }
  JLA_DEV void unpack(uint32_t u, uint32_t& key, float& x) const { key = u, x = kfloat(u); }
};
// typical: over S2, by the distance d = |(m - l) - h| ascending
struct NsTypicalKey {
  NsRow r;
  NsKeep keep;
  float h;
  JLA_DEV bool in(int i, float x) const { return keep(fkey(x), i); }
  JLA_DEV uint32_t key(float x) const {
    return ~__float_as_uint(fabsf(__fadd_rn(__fsub_rn(ns_l(r, x), r.m), h)));
  }
  JLA_DEV uint32_t pack(float x, uint32_t) const { return __float_as_uint(x); }
  JLA_DEV void unpack(uint32_t u, uint32_t& key, float& x) const { x = __uint_as_float(u), key = this->key(x); }
};

// Wave 0 scans bins nb-1 .. 0: the boundary bin of the count target kr (first bin at which the cumulative count
// reaches kr) or of the mass target tr (first at which the cumulative mass reaches tr). frac > 0: tr is not known yet
// and becomes ceil(frac * total mass), in fp64. Writes sh.sel_*.
JLA_DEV void ns_scan_bins(NsShared& sh, int nb, bool by_mass, uint32_t kr, u64_t tr, double frac) {
  if (threadIdx.x >= 64) return;
  const int l = threadIdx.x, per = nb / 64;
  uint32_t sc = 0;
  u64_t sm = 0;
  for (int q = 0; q < per; ++q) {  // lane l owns bins nb-1 - l*per .. (descending)
    sc += sh.cnt[nb - 1 - (l * per + q)];
    sm += sh.mass[nb - 1 - (l * per + q)];
  }
  uint32_t ic = sc;
  u64_t im = sm;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t tc = __shfl_up(ic, o, 64);
    const u64_t tm = __shfl_up(im, o, 64);
    if (l >= o) ic += tc, im += tm;
  }
  const u64_t tot_m = __shfl(im, 63, 64);
  if (by_mass) {
    if (frac > 0.0) tr = (u64_t)ceil((double)tot_m * frac);
    tr = min(max(tr, (u64_t)1), tot_m);
  }
  uint32_t ac = ic - sc;
  u64_t am = im - sm;
  if (by_mass ? (am < tr && tr <= im) : (ac < kr && kr <= ic)) {  // exactly one lane
    for (int q = 0; q < per; ++q) {
      const int bin = nb - 1 - (l * per + q);
      const uint32_t c = sh.cnt[bin];
      const u64_t mm = sh.mass[bin];
      if (by_mass ? tr <= am + mm : kr <= ac + c) {
        sh.sel_bin = bin, sh.sel_above_c = ac, sh.sel_bin_c = c;
        sh.sel_above_m = am, sh.sel_bin_m = mm;
        break;
      }
      ac += c, am += mm;
    }
  }
  if (l == 0) sh.sel_tr = tr;
}

// a thread's pending histogram update: consecutive keys of one bin cost one pair of atomics
struct NsAcc {
  int bin = -1;
  uint32_t c = 0;
  u64_t m = 0;
};
JLA_DEV void ns_flush(NsShared& sh, NsAcc& a, bool with_mass) {
  if (a.bin >= 0) {
    atomicAdd(&sh.cnt[a.bin], a.c);
    if (with_mass) atomicAdd(&sh.mass[a.bin], a.m);
  }
}

struct NsCut {
  uint32_t T, n_eq, c_eq, kept;  // survivors: key > T and the first n_eq of the c_eq keys == T; kept of them in all
  u64_t z;                       // count descent: the survivors' mass
  u64_t tr;                      // mass descent: what of the target is left for the keys == T
  uint32_t n_list;               // > 0: the LDS list holds the first pass's boundary bin
};

// BY_MASS false: the k largest keys (with_mass: also their mass, in z). BY_MASS true: the ranks with less than
// ceil(top_p * Z) of mass before them, Z = z_known or (0) the row's total. kf: the order and the tokens it ranges over.
template <bool BY_MASS, typename K>
JLA_DEV NsCut ns_descend(const K& kf, const NsRow& r, NsShared& sh, bool with_mass, uint32_t k, double top_p,
                         u64_t z_known) {
  uint32_t prefix = 0, mask = 0, kr = k, acc_c = 0, bin_c = 0, n_list = 0;
  u64_t tr = BY_MASS && z_known ? (u64_t)ceil((double)z_known * top_p) : 0, acc_m = 0, bin_m = 0;
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0, nb = pass == 2 ? 1024 : NS_BINS;
    for (int i = threadIdx.x; i < nb; i += NS_THREADS) sh.cnt[i] = 0, sh.mass[i] = 0;
    __syncthreads();
    NsAcc acc;
    auto add = [&](uint32_t key, float x) {
      if ((key & mask) != prefix) return;
      const int bin = (key >> shift) & (nb - 1);
      if (bin != acc.bin) {
        ns_flush(sh, acc, with_mass);
        acc.bin = bin, acc.c = 0, acc.m = 0;
      }
      ++acc.c;
      if (with_mass) acc.m += ns_mass(r, x);
    };
    if (n_list) {
      for (int j = threadIdx.x; j < (int)n_list; j += NS_THREADS) {
        uint32_t key;
        float x;
        kf.unpack(sh.lkey[j], key, x);
        add(key, x);
      }
    } else {
      for (int i4 = threadIdx.x; i4 < r.n4; i4 += NS_THREADS) {
        float v[4];
        const int n = ns_load4(r, i4, v);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q < n && kf.in(4 * i4 + q, v[q])) add(kf.key(v[q]), v[q]);
      }
    }
    ns_flush(sh, acc, with_mass);
    __syncthreads();
    ns_scan_bins(sh, nb, BY_MASS, kr, tr, BY_MASS && pass == 0 && !z_known ? top_p : 0.0);
    __syncthreads();
    prefix |= sh.sel_bin << shift;
    mask |= (uint32_t)(nb - 1) << shift;
    acc_c += sh.sel_above_c, acc_m += sh.sel_above_m;
    kr -= sh.sel_above_c;
    if (BY_MASS) tr = sh.sel_tr - sh.sel_above_m;
    bin_c = sh.sel_bin_c, bin_m = sh.sel_bin_m;
    __syncthreads();
    if (pass == 0 && bin_c <= (uint32_t)NS_CAP) {  // compact the boundary bin, in index order
      uint32_t base = 0;
      for (int t0 = 0; t0 < r.n4; t0 += NS_THREADS) {
        const int i4 = t0 + threadIdx.x;
        float v[4];
        const int n = i4 < r.n4 ? ns_load4(r, i4, v) : 0;
        uint32_t key[4], c = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          key[q] = q < n && kf.in(4 * i4 + q, v[q]) ? kf.key(v[q]) : ~prefix;  // (~prefix never matches)
          c += (key[q] & mask) == prefix;
        }
        uint32_t tot;
        uint32_t pos = base + ns_block_scan(c, sh, tot);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if ((key[q] & mask) == prefix && pos < (uint32_t)NS_CAP) {
            sh.lkey[pos] = kf.pack(v[q], key[q]);
            sh.lidx[pos] = 4 * i4 + q;
            ++pos;
          }
        base += tot;
      }
      n_list = bin_c;
      __syncthreads();
    }
  }
  NsCut cut;
  cut.T = prefix, cut.c_eq = bin_c, cut.n_list = n_list, cut.tr = tr;
  const u64_t mu = bin_m / max(bin_c, 1u);  // the keys of the last bin are equal, and so are their masses
  if (BY_MASS) {
    cut.n_eq = mu ? (uint32_t)min((u64_t)bin_c, (tr + mu - 1) / mu) : bin_c;
    cut.kept = acc_c + cut.n_eq;
    cut.z = 0;
  } else {
    cut.n_eq = kr;
    cut.kept = k;
    cut.z = acc_m + kr * mu;
  }
  return cut;
}

// The vocabulary index of the n_eq-th key == T in index order. get(g, key, idx) yields group g's (up to four)
// consecutive entries and returns how many.
template <typename G>
JLA_DEV int32_t ns_nth_tie(NsShared& sh, int ngroups, uint32_t T, uint32_t n_eq, G&& get) {
  uint32_t seen = 0;
  if (threadIdx.x == 0) sh.tie_idx = 0x7fffffff;  // (the scan's barriers order this before the write below)
  for (int t0 = 0; t0 < ngroups && seen < n_eq; t0 += NS_THREADS) {  // seen is uniform: so is the trip count
    uint32_t key[4], c = 0;
    int32_t idx[4];
    const int n = t0 + (int)threadIdx.x < ngroups ? get(t0 + (int)threadIdx.x, key, idx) : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) c += q < n && key[q] == T;
    uint32_t tot;
    uint32_t ex = seen + ns_block_scan(c, sh, tot);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < n && key[q] == T) {
        if (ex == n_eq - 1) sh.tie_idx = idx[q];
        ++ex;
      }
    seen += tot;
  }
  __syncthreads();
  return sh.tie_idx;
}

// typical's tie group, whose masses may differ: the vocabulary index of the first key == T, in index order, at which
// the group's cumulative mass reaches tr (1 <= tr <= the group's mass). get(g, hit, idx, ms) yields group g's entries,
// hit = "takes part and key == T", and returns how many. (Unequal masses inside a tie group come only from two fp32
// distances that round to the same bits on either side of h: no exact-grid row has them, and no test does.)
template <typename G>
JLA_DEV int32_t ns_mass_tie(NsShared& sh, int ngroups, u64_t tr, G&& get) {
  u64_t seen = 0;
  if (threadIdx.x == 0) sh.tie_idx = 0x7fffffff;
  for (int t0 = 0; t0 < ngroups && seen < tr; t0 += NS_THREADS) {  // seen is uniform: so is the trip count
    bool hit[4] = {};
    int32_t idx[4] = {};
    u64_t ms[4] = {}, c = 0;
    const int n = t0 + (int)threadIdx.x < ngroups ? get(t0 + (int)threadIdx.x, hit, idx, ms) : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      hit[q] = q < n && hit[q];
      c += hit[q] ? ms[q] : 0;
    }
    u64_t tot;
    u64_t ex = seen + ns_block_scan(c, sh, tot);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (hit[q]) {
        if (ex < tr && tr <= ex + ms[q]) sh.tie_idx = idx[q];  // exactly one entry of the group
        ex += ms[q];
      }
    seen += tot;
  }
  __syncthreads();
  return sh.tie_idx;
}

// min_p as a bound on the key: the smallest key whose mass reaches min_mass (the row maximum's, 2^40, always does).
// The bisection takes ns_mass to be monotone in the key; the device's exp2f is not formally so, and a local inversion
// would put kmin a key ulp or two beside the per-token test mass >= min_mass (far inside the definition's rounding).
JLA_DEV uint32_t ns_min_key(const NsRow& r, uint32_t kmax, u64_t min_mass) {
  uint32_t lo = fkey(-INFINITY), hi = kmax;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (ns_mass(r, kfloat(mid)) >= min_mass) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// -log(-log(u)), u = (n + 0.5) / 2^24 with n = the word's top 24 bits. Both branches feed exact fp32 arguments: the
// upper half of the range goes through log1p(-(1 - u)), where the winners of a long row live (u within 1e-5 of 1).
JLA_DEV float ns_gumbel(uint32_t w) {
  const uint32_t n = w >> 8;
  const float a = n < (1u << 23) ? -logf(((float)n + 0.5f) * (1.0f / 16777216.0f))
                                 : -log1pf(-(float)((1u << 25) - 2u * n - 1u) * (1.0f / 33554432.0f));
  return -logf(a);
}

// MINP: min_mass > 0 is the min_p cut. TYP: typical_p < 1 is the typical cut.
template <bool MINP, bool TYP>
__global__ void __launch_bounds__(NS_THREADS)
    nucleus_sample_kernel(const float* __restrict__ logits, int V, int k, float inv_t, double top_p, int vec,
                          uint32_t seed_lo, uint32_t seed_hi, const int32_t* __restrict__ step,
                          int32_t* __restrict__ nxt, int32_t* __restrict__ kept, u64_t min_mass, double typical_p) {
  __shared__ NsShared sh;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  NsRow r;
  r.x = logits + (size_t)b * V;
  r.V = V, r.n4 = (V + 3) >> 2, r.vec = vec != 0, r.inv_t = inv_t;

  // sweep 1: the row maximum, as a key
  uint32_t kmax = 0;
  for (int i4 = threadIdx.x; i4 < r.n4; i4 += NS_THREADS) {
    float v[4];
    const int n = ns_load4(r, i4, v);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < n) kmax = max(kmax, fkey(v[q]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor(kmax, o, 64));
  if (lane == 0) sh.red_k[wave] = kmax;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NS_WAVES; ++i) kmax = max(kmax, sh.red_k[i]);
  r.dead = kmax <= fkey(-INFINITY);
  r.m = r.dead ? 0.f : __fmul_rn(kfloat(kmax), inv_t);

  const bool use_k = k < V, use_p = top_p < 1.0;
  bool all = !use_k && !use_p;
  uint32_t T = 0, n_kept = (uint32_t)V;
  int32_t tie_idx = 0x7fffffff;
  if (!all) {
    NsCut cut;
    if (use_k) cut = ns_descend<false>(NsLogitKey{}, r, sh, use_p, (uint32_t)k, 0.0, 0);
    if (use_p) cut = ns_descend<true>(NsLogitKey{}, r, sh, true, 0, top_p, use_k ? cut.z : 0);
    T = cut.T, n_kept = cut.kept;
    if (cut.n_eq < cut.c_eq) {
      if (cut.n_list)
        tie_idx = ns_nth_tie(sh, ((int)cut.n_list + 3) >> 2, T, cut.n_eq,
                             [&](int g, uint32_t(&key)[4], int32_t(&idx)[4]) {
          const int n = min(4, (int)cut.n_list - 4 * g);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q < n) key[q] = sh.lkey[4 * g + q], idx[q] = sh.lidx[4 * g + q];
          return n;
        });
      else
        tie_idx = ns_nth_tie(sh, r.n4, T, cut.n_eq, [&](int g, uint32_t(&key)[4], int32_t(&idx)[4]) {
          float v[4];
          const int n = ns_load4(r, g, v);
#pragma unroll
          for (int q = 0; q < 4; ++q) key[q] = fkey(v[q]), idx[q] = 4 * g + q;
          return n;
        });
    }
  }
  const NsKeep keep{all, T, MINP ? ns_min_key(r, kmax, min_mass) : 0u, tie_idx};

  // typical: Z2 and W over S2 give h; then the mass descent on the distance key, and the cut inside its tie group
  NsTypicalKey tk{r, keep, 0.f};
  uint32_t Td = 0;
  int32_t tie_d = 0x7fffffff;
  if (TYP) {
    if (threadIdx.x == 0) sh.z2 = 0, sh.w = 0;
    __syncthreads();
    u64_t z = 0, w = 0;
    for (int i4 = threadIdx.x; i4 < r.n4; i4 += NS_THREADS) {
      float v[4];
      const int n = ns_load4(r, i4, v);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (!(q < n && keep(fkey(v[q]), 4 * i4 + q))) continue;
        const u64_t mass = ns_mass(r, v[q]);
        if (mass) z += mass, w += (u64_t)((double)mass * (double)__fsub_rn(r.m, ns_l(r, v[q])));  // (mass 0: l = -inf)
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64), w += __shfl_xor(w, o, 64);
    if (lane == 0) atomicAdd(&sh.z2, z), atomicAdd(&sh.w, w);
    __syncthreads();
    tk.h = (float)((double)sh.w / (double)sh.z2);
    const NsCut cut = ns_descend<true>(tk, r, sh, true, 0, typical_p, sh.z2);
    Td = cut.T;
    if (cut.c_eq > 1) {
      if (cut.n_list)
        tie_d = ns_mass_tie(sh, ((int)cut.n_list + 3) >> 2, cut.tr,
                            [&](int g, bool(&hit)[4], int32_t(&idx)[4], u64_t(&ms)[4]) {
          const int n = min(4, (int)cut.n_list - 4 * g);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q < n) {
              const float x = __uint_as_float(sh.lkey[4 * g + q]);
              hit[q] = tk.key(x) == Td, idx[q] = sh.lidx[4 * g + q], ms[q] = ns_mass(r, x);
            }
          return n;
        });
      else
        tie_d = ns_mass_tie(sh, r.n4, cut.tr, [&](int g, bool(&hit)[4], int32_t(&idx)[4], u64_t(&ms)[4]) {
          float v[4];
          const int n = ns_load4(r, g, v);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            hit[q] = tk.in(4 * g + q, v[q]) && tk.key(v[q]) == Td, idx[q] = 4 * g + q, ms[q] = ns_mass(r, v[q]);
          return n;
        });
    }
  }

  // draw: Gumbel-max over the survivors, noise keyed by the vocabulary index
  const uint32_t st = (uint32_t)step[0];
  float best = -INFINITY;
  int32_t bi = 0x7fffffff;
  uint32_t drawn = 0;  // (MINP or TYP) the survivors, counted where they are scored
  for (int i4 = threadIdx.x; i4 < r.n4; i4 += NS_THREADS) {
    float v[4];
    const int n = ns_load4(r, i4, v);
    bool s[4], any = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t key = fkey(v[q]);
      s[q] = q < n && (all || key > T || (key == T && 4 * i4 + q <= tie_idx));  // (keep, written out)
      if (MINP) s[q] = s[q] && key >= keep.kmin;
      if (TYP) {
        const uint32_t dk = tk.key(v[q]);
        s[q] = s[q] && (dk > Td || (dk == Td && 4 * i4 + q <= tie_d));
      }
      if (MINP || TYP) drawn += s[q];
      any |= s[q];
    }
    if (!any) continue;
    const uint4 w4 = philox4x32_10(make_uint4((uint32_t)i4, (uint32_t)b, st, 1u), make_uint2(seed_lo, seed_hi));
    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!s[q]) continue;
      const float score = __fadd_rn(ns_l(r, v[q]), ns_gumbel(w[q]));
      if (score > best) best = score, bi = 4 * i4 + q;  // ascending index within a thread: the first maximum stays
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(best, o, 64);
    const int32_t oi = __shfl_xor(bi, o, 64);
    if (os > best || (os == best && oi < bi)) best = os, bi = oi;
  }
  if (MINP || TYP) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) drawn += __shfl_xor(drawn, o, 64);
    if (lane == 0) sh.red_c[wave] = drawn;
  }
  if (lane == 0) sh.red_s[wave] = best, sh.red_i[wave] = bi;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < NS_WAVES; ++i)
      if (sh.red_s[i] > best || (sh.red_s[i] == best && sh.red_i[i] < bi)) best = sh.red_s[i], bi = sh.red_i[i];
    nxt[b] = min(bi, V - 1);  // (a row outside the contract, NaN throughout, still yields a token of the vocabulary)
    if (MINP || TYP) {
      n_kept = 0;
      for (int i = 0; i < NS_WAVES; ++i) n_kept += sh.red_c[i];
    }
    if (kept) kept[b] = (int32_t)n_kept;
  }
}

}  // namespace

int nucleus_sample_max_v() { return NS_MAX_V; }

int nucleus_sample(const float* logits, int B, int V, int top_k, double temperature, double top_p, uint64_t seed,
                   const int32_t* step, int32_t* nxt, int32_t* kept, double min_p, double typical_p, hipStream_t s) {
  if (B <= 0) return 0;
  if (V < 1 || V > NS_MAX_V || top_k < 0) return -1;
  if (!logits || !step || !nxt || !(temperature > 0.0) || !(top_p > 0.0)) return -2;
  if (!(min_p >= 0.0 && min_p <= 1.0) || !(typical_p > 0.0 && typical_p <= 1.0)) return -2;
  const int k = top_k == 0 ? V : min(top_k, V);
  const int vec = (V & 3) == 0 && V >= 1024 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
  const float inv_t = (float)(1.0 / temperature);  // fp64, rounded once (process_logits' convention)
  const u64_t min_mass = (u64_t)ceil(min_p * 1099511627776.0);  // 0: no min_p cut
  const bool typ = typical_p < 1.0;
  auto* kern = min_mass ? (typ ? nucleus_sample_kernel<true, true> : nucleus_sample_kernel<true, false>)
                        : (typ ? nucleus_sample_kernel<false, true> : nucleus_sample_kernel<false, false>);
  kern<<<B, NS_THREADS, 0, s>>>(logits, V, k, inv_t, top_p, vec, (uint32_t)seed, (uint32_t)(seed >> 32), step, nxt,
                                kept, min_mass, typical_p);
  JLA_CHECK_LAUNCH();
  return 0;
}

}  // namespace jla
