// Local 3D geometry statistics of decoded molecules on the device: bond lengths, bond angles and dihedral angles, histogrammed per
// bond pattern.  It stands in, without RDKit, for the reference's Local3D (utils/evaluation.py:156-329): there a pattern is a linear
// SMARTS such as c:c, [#6]-[#7]-[#6] or c:c:c:c matched with uniquify = True; here it is the chain (element, bond type, element, ...)
// of class indices and bond type ids, and the molecule is the one the decode wrote, not RDKit's reconstruction of it.
//
// One workgroup of 256 threads per molecule over the compact arrays of mdx_mol.h, with a position per compact atom beside them.
//
// Items.  A length item is a bond (i, j).  An angle item is a centre b with two bond entries to neighbours a < c.  A dihedral item is
// a central bond (b, c), visited once, with a bond entry b-a (a != c) and a bond entry c-d (d != b, d != a): all four atoms distinct
// (a = d closes a triangle and is no dihedral), and a path and its reverse are one item.  Bonds with an index outside the molecule or
// with i = j are ignored everywhere.
//
// Patterns.  An item's chain and its reverse are each packed into a 64-bit key, one byte per field with the first field on top, so
// that comparing keys is comparing chains lexicographically; the smaller key is looked up among the kind's rows (the launch wrapper
// canonicalises the rows the same way).  A class or bond id outside its range packs as 0xff, which no row holds.
//
// Adjacency.  cur[i] = degree (atomic adds) -> exclusive scan -> each bond claims a slot at both ends with a returning atomic add,
// after which cur[i] is the END of atom i's list and the start is cur[i - 1].  A list entry is (bond key << 24) | neighbour.  The
// slot order depends on the order the atomics land in; every output is a count, so nothing else does.  cur, the lists, the element
// keys and the positions live in LDS for a molecule of at most L3_LDS_ATOMS atoms and L3_LDS_BONDS bonds, else cur and the lists live
// in the caller's workspace: the same code walks either (generic pointers).  What atomics update in global memory is read back with
// agent-scope loads.
//
// Histograms.  Bin = (int)((v - lo) * n / (hi - lo)), the last bin closed; a value outside [lo, hi], NaN included, counts in
// outside[row].  With at most L3_LDS_BINS bins over all rows the workgroup counts in LDS (uint32) and adds its non-zero bins to the
// global int64 table with one atomic each, else every item adds to the global table directly.  Integer adds: both are exact.
#include "mdx_kernels.h"

namespace {

constexpr float L3_DEG = 57.29577951308232f;  // 180 / pi, rounded to fp32

struct V3 {
  float x, y, z;
};
// coordinate differences as dist3 (mdx_molcheck.hip) forms them; every operation below is rounded to fp32 on its own
__device__ inline V3 diff3(const float* p, int a, int b) {
#pragma clang fp contract(off)
  return {p[3 * (size_t)a + 0] - p[3 * (size_t)b + 0], p[3 * (size_t)a + 1] - p[3 * (size_t)b + 1],
          p[3 * (size_t)a + 2] - p[3 * (size_t)b + 2]};
}
__device__ inline float dot3(V3 u, V3 v) {
#pragma clang fp contract(off)
  return u.x * v.x + u.y * v.y + u.z * v.z;
}
__device__ inline V3 cross3(V3 u, V3 v) {
#pragma clang fp contract(off)
  return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}
__device__ inline float angle_deg(const float* p, int a, int b, int c) {
#pragma clang fp contract(off)
  const V3 u = diff3(p, a, b), v = diff3(p, c, b), w = cross3(u, v);
  return atan2f(sqrtf(dot3(w, w)), dot3(u, v)) * L3_DEG;
}
__device__ inline float dihedral_deg(const float* p, int a, int b, int c, int d) {
#pragma clang fp contract(off)
  const V3 b1 = diff3(p, b, a), b2 = diff3(p, c, b), b3 = diff3(p, d, c);
  const V3 n1 = cross3(b1, b2), n2 = cross3(b2, b3), m = cross3(n1, n2);
  return atan2f(dot3(m, b2) / sqrtf(dot3(b2, b2)), dot3(n1, n2)) * L3_DEG;
}

__global__ __launch_bounds__(256) void mol_local3d_kernel(const Local3DArgs A) {
  __shared__ unsigned long long s_key[3 * L3_MAX_ROWS];
  __shared__ unsigned s_hist[L3_LDS_BINS];
  __shared__ unsigned s_out[3 * L3_MAX_ROWS];
  __shared__ int s_adj[2 * L3_LDS_BONDS];
  __shared__ int s_cur[L3_LDS_ATOMS];
  __shared__ float s_pos[3 * L3_LDS_ATOMS];
  __shared__ unsigned char s_el[L3_LDS_ATOMS];
  __shared__ unsigned long long s_items[3];
  __shared__ int s_wsum[4];
  __shared__ int s_carry;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long* items_out = A.n_items + m;  // (3, B)
  const MolView v = mol_view(A.mol, m);
  const long long n0 = v.n0, h0 = v.h0;
  const int n = v.n, nb = v.nb;
  if (v.masked || v.outside) {  // uniform: the molecule contributes nothing
    if (tid < 3) items_out[(size_t)tid * A.B] = 0;
    return;
  }
  const int P = A.kptr[3];
  const bool small = n <= L3_LDS_ATOMS && nb <= L3_LDS_BONDS;
  int* cur = small ? s_cur : A.ws_cur + n0;
  int* adj = small ? s_adj : A.ws_adj + 2 * h0;
  const float* pos = small ? s_pos : A.atom_pos + 3 * (size_t)n0;
  const int* atype = A.mol.atom_type + n0;
  const int *bi = A.mol.bond_i + h0, *bj = A.mol.bond_j + h0, *bt = A.mol.bond_type + h0;
  const unsigned num_element = A.num_element, num_bond_types = A.num_bond_types;
  auto el = [&](int i) -> unsigned long long {
    if (small) return s_el[i];
    const unsigned t = (unsigned)atype[i];
    return t < num_element ? t : 0xffu;
  };
  auto bkey = [&](int t) -> unsigned { return (unsigned)(t - 1) < num_bond_types ? (unsigned)t : 0xffu; };

  for (int r = tid; r < P; r += 256) {
    s_key[r] = A.keys[r];
    s_out[r] = 0u;
  }
  if (A.lds_hist)
    for (int k = tid; k < (int)A.total_bins; k += 256) s_hist[k] = 0u;
  for (int i = tid; i < n; i += 256) {
    st(&cur[i], 0);
    if (small) {
      const unsigned t = (unsigned)atype[i];
      s_el[i] = (unsigned char)(t < num_element ? t : 0xffu);
      s_pos[3 * i + 0] = A.atom_pos[3 * (size_t)(n0 + i) + 0];
      s_pos[3 * i + 1] = A.atom_pos[3 * (size_t)(n0 + i) + 1];
      s_pos[3 * i + 2] = A.atom_pos[3 * (size_t)(n0 + i) + 2];
    }
  }
  if (tid < 3) s_items[tid] = 0ull;
  if (tid == 0) s_carry = 0;
  __syncthreads();

  // ---- adjacency: degrees -> exclusive scan -> fill -------------------------------------------------------------------------------
  for (int b = tid; b < nb; b += 256) {
    const int i = bi[b], j = bj[b];
    if (!mol_bond_ok(i, j, n)) continue;
    atomicAdd(&cur[i], 1);
    atomicAdd(&cur[j], 1);
  }
  __syncthreads();
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int i = c0 + tid;
    const int d = i < n ? ld(&cur[i]) : 0;
    const int incl = wave_inclusive_scan(d);
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int off = s_carry;
    for (int w = 0; w < wave; ++w) off += s_wsum[w];
    if (i < n) st(&cur[i], off + incl - d);
    __syncthreads();
    if (tid == 0) s_carry += s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
    __syncthreads();
  }
  for (int b = tid; b < nb; b += 256) {
    const int i = bi[b], j = bj[b];
    if (!mol_bond_ok(i, j, n)) continue;
    const int k = (int)(bkey(bt[b]) << 24);
    st(&adj[atomicAdd(&cur[i], 1)], k | j);  // slots stay below 2 * (valid bonds) <= 2 * nb: the degrees counted the same bonds
    st(&adj[atomicAdd(&cur[j], 1)], k | i);
  }
  __syncthreads();
  auto first = [&](int i) { return i ? ld(&cur[i - 1]) : 0; };

  // ---- one item: look its key up among the kind's rows; only a hit pays for the value, which is then binned ------------------------
  auto find = [&](int kind, unsigned long long fwd, unsigned long long rev) -> int {
    const unsigned long long key = fwd < rev ? fwd : rev;
    for (int r = A.kptr[kind]; r < A.kptr[kind + 1]; ++r)
      if (s_key[r] == key) return r;
    return -1;
  };
  auto tally = [&](int kind, int row, float v) {
    const float lo = A.lo[kind], hi = A.hi[kind];
    if (!(v >= lo && v <= hi)) {  // NaN fails both
      atomicAdd(&s_out[row], 1u);
      return;
    }
    float t;
    {
#pragma clang fp contract(off)
      t = (v - lo) * A.scale[kind];
    }
    const int nbin = A.nbins[kind];
    const int bin = (int)fminf(t, (float)(nbin - 1));
    const size_t idx = (size_t)A.hoff[kind] + (size_t)(row - A.kptr[kind]) * (size_t)nbin + (size_t)bin;
    if (A.lds_hist)
      atomicAdd(&s_hist[idx], 1u);
    else
      atomicAdd(&A.hist[idx], 1ull);
  };

  unsigned long long cnt_len = 0, cnt_ang = 0, cnt_dih = 0;
  for (int b = tid; b < nb; b += 256) {
    const int i = bi[b], j = bj[b];
    if (!mol_bond_ok(i, j, n)) continue;
    const unsigned long long ei = el(i), ej = el(j), t = bkey(bt[b]);
    // ---- length -------------------------------------------------------------------------------------------------------------------
    ++cnt_len;
    const int row_len = find(0, ei << 16 | t << 8 | ej, ej << 16 | t << 8 | ei);
    if (row_len >= 0) {
      const V3 d = diff3(pos, i, j);
      float len;
      {
#pragma clang fp contract(off)
        len = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
      }
      tally(0, row_len, len);
    }
    // ---- angles: this bond as the leg a - centre, from both ends; the other leg goes to a neighbour c > a -------------------------
    for (int side = 0; side < 2; ++side) {
      const int ctr = side ? j : i, a = side ? i : j;
      const unsigned long long ec = side ? ej : ei, ea = side ? ei : ej;
      const int s1 = ld(&cur[ctr]);
      for (int s = first(ctr); s < s1; ++s) {
        const int e = ld(&adj[s]), c = e & 0xffffff;
        if (c <= a) continue;
        ++cnt_ang;
        if (A.kptr[2] == A.kptr[1]) continue;
        const unsigned long long t2 = (unsigned)e >> 24, ecc = el(c);
        const int row = find(1, ea << 32 | t << 24 | ec << 16 | t2 << 8 | ecc, ecc << 32 | t2 << 24 | ec << 16 | t << 8 | ea);
        if (row >= 0) tally(1, row, angle_deg(pos, a, ctr, c));
      }
    }
    // ---- dihedrals: this bond as the central bond i - j ---------------------------------------------------------------------------
    const int si1 = ld(&cur[i]), sj0 = first(j), sj1 = ld(&cur[j]);
    for (int s = first(i); s < si1; ++s) {
      const int e1 = ld(&adj[s]), a = e1 & 0xffffff;
      if (a == j) continue;
      const unsigned long long t1 = (unsigned)e1 >> 24, ea = el(a);
      for (int q = sj0; q < sj1; ++q) {
        const int e3 = ld(&adj[q]), d = e3 & 0xffffff;
        if (d == i || d == a) continue;
        ++cnt_dih;
        if (A.kptr[3] == A.kptr[2]) continue;
        const unsigned long long t3 = (unsigned)e3 >> 24, ed = el(d);
        const int row = find(2, ea << 48 | t1 << 40 | ei << 32 | t << 24 | ej << 16 | t3 << 8 | ed,
                             ed << 48 | t3 << 40 | ej << 32 | t << 24 | ei << 16 | t1 << 8 | ea);
        if (row >= 0) tally(2, row, dihedral_deg(pos, a, i, j, d));
      }
    }
  }
  if (cnt_len) atomicAdd(&s_items[0], cnt_len);
  if (cnt_ang) atomicAdd(&s_items[1], cnt_ang);
  if (cnt_dih) atomicAdd(&s_items[2], cnt_dih);
  __syncthreads();
  if (tid < 3) items_out[(size_t)tid * A.B] = (long long)s_items[tid];
  for (int r = tid; r < P; r += 256)
    if (s_out[r]) atomicAdd(&A.outside[r], (unsigned long long)s_out[r]);
  if (A.lds_hist)
    for (int k = tid; k < (int)A.total_bins; k += 256)
      if (s_hist[k]) atomicAdd(&A.hist[k], (unsigned long long)s_hist[k]);
}

}  // namespace

void launch_mol_local3d(const Local3DArgs& a, hipStream_t s) {
  if (a.B > 0) hipLaunchKernelGGL(mol_local3d_kernel, dim3(a.B), dim3(256), 0, s, a);
}
