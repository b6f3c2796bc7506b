// Quality check of the decoded molecules on the device, right after mdx_decode_output (mdx_decode.hip): per molecule the
// fragments of its bond graph, its atoms' valences against a caller-supplied table, its shortest inter-atomic distance and its
// longest bond; optionally the restriction of a molecule to one fragment.  It stands in for the reference's "finished" test
// (scripts/sample_drug3d.py:141-153: RDKit sanitises the molecule and its SMILES has no '.') as far as that goes without RDKit:
// connectivity is the same test, the valence rule is a NECESSARY condition of Chem.SanitizeMol (utils/reconstruct.py:245-271) --
// no kekulisation, no aromaticity perception, no charges.
//
// Both kernels read the COMPACT arrays mdx_decode_output leaves at each molecule's original offsets (atoms at node_ptr[m] ..
// + n_atoms[m], bonds at he_ptr[m] .. + n_bonds[m], one direction per bond, molecule-local atom indices), one workgroup of 256
// threads per molecule.
//
// Fragment labelling: lab[i] starts as i.  One sweep = (a) every bond (i, j) lowers lab[i] and lab[j] to min(lab[i], lab[j]) with
// atomicMin, (b) every atom lowers lab[i] to lab[lab[i]] (pointer jumping).  At every moment lab[i] is the index of an atom of i's
// fragment and lab[i] <= i, and labels only fall, so whatever order the atomics land in, the only state no sweep changes is
// lab[i] = smallest index of i's fragment: the result does not depend on update order.  Step (a) alone moves the smallest index
// of a fragment at least one bond further per sweep, so a molecule of n atoms is done after at most n - 1 changing sweeps (+ 1
// that sees no change); (b) can only lower labels further, so it shortens that and never lengthens it (long chains in shuffled
// numbering collapse by pointer jumping instead of one bond per sweep).  The loop is bounded by n sweeps as well as by the
// no-change flag.  All other reductions are integer sums or min / max, which are
// order-independent too, so every output is bit-reproducible and independent of where the molecule sits in the batch.
#include "mdx_kernels.h"

namespace {

constexpr int MC_LDS_ATOMS = 512;  // molecules up to this size keep labels / fragment sizes / valences in LDS (6 KB)

// |a - b| exactly as the documents state it: three subtractions, three squares, two adds, one square root, each rounded to fp32
__device__ inline float dist3(const float* __restrict__ p, int a, int b) {
#pragma clang fp contract(off)
  const float dx = p[3 * (size_t)a + 0] - p[3 * (size_t)b + 0];
  const float dy = p[3 * (size_t)a + 1] - p[3 * (size_t)b + 1];
  const float dz = p[3 * (size_t)a + 2] - p[3 * (size_t)b + 2];
  return sqrtf(dx * dx + dy * dy + dz * dz);
}

// Labels, fragment sizes and valences are updated with atomics, which a large molecule's global-memory arrays see in L2: they
// are read back with the agent-scope ld / st of mdx_mol.h so that no read is served from a stale line of the CU's vector L1.

__global__ __launch_bounds__(256) void mol_check_kernel(
    const int* __restrict__ node_ptr, const int* __restrict__ he_ptr, const int* __restrict__ atom_type,
    const float* __restrict__ atom_pos, const int* __restrict__ n_atoms, const int* __restrict__ bond_type,
    const int* __restrict__ bond_i, const int* __restrict__ bond_j, const int* __restrict__ n_bonds,
    const int* __restrict__ max_valence, int num_element, int num_bond_types, int* ws_lab, int* ws_cnt,
    int* __restrict__ component, int* __restrict__ valence2, int* __restrict__ n_components, int* __restrict__ largest_size,
    int* __restrict__ largest_label, int* __restrict__ n_overvalent, float* __restrict__ min_dist,
    float* __restrict__ max_bond_len) {
  __shared__ int s_lab[MC_LDS_ATOMS], s_cnt[MC_LDS_ATOMS], s_val[MC_LDS_ATOMS];
  __shared__ int s_changed, s_ncomp, s_over;
  __shared__ unsigned s_dmin, s_bmax;            // bit patterns of non-negative floats order like the floats
  __shared__ unsigned long long s_best;          // (size << 32) | (INT_MAX - label): max = largest, ties to the smaller label
  const int m = blockIdx.x, tid = threadIdx.x;
  const int n0 = node_ptr[m], h0 = he_ptr[m], n = n_atoms[m], nb = n_bonds[m];
  const bool small = n <= MC_LDS_ATOMS;
  // the same code walks LDS or global memory (generic pointers); a large molecule keeps its valences in the output array itself
  int* lab = small ? s_lab : ws_lab + n0;
  int* cnt = small ? s_cnt : ws_cnt + n0;
  int* val = small ? s_val : valence2 + n0;
  const float* pos = atom_pos + 3 * (size_t)n0;
  for (int i = tid; i < n; i += 256) {
    st(&lab[i], i);
    st(&cnt[i], 0);
    st(&val[i], 0);
  }
  if (tid == 0) {
    s_ncomp = 0;
    s_over = 0;
    s_dmin = 0x7f800000u;  // +inf
    s_bmax = 0u;
    s_best = 0ull;
  }
  __syncthreads();
  // ---- valences and the longest bond: one pass over the bonds ---------------------------------------------------------------
  for (int b = tid; b < nb; b += 256) {
    const int i = bond_i[h0 + b], j = bond_j[h0 + b], t = bond_type[h0 + b];
    if ((unsigned)i >= (unsigned)n || (unsigned)j >= (unsigned)n) continue;  // never from mdx_decode_output; keeps accesses in bounds
    const int w = (t == num_bond_types) ? 3 : 2 * t;                         // twice the bond order; the last type is aromatic (1.5)
    atomicAdd(&val[i], w);
    atomicAdd(&val[j], w);
    atomicMax(&s_bmax, __float_as_uint(dist3(pos, i, j)));
  }
  // ---- fragments ------------------------------------------------------------------------------------------------------------
  for (int sweep = 0; sweep < n; ++sweep) {
    if (tid == 0) s_changed = 0;
    __syncthreads();
    bool ch = false;
    for (int b = tid; b < nb; b += 256) {
      const int i = bond_i[h0 + b], j = bond_j[h0 + b];
      if ((unsigned)i >= (unsigned)n || (unsigned)j >= (unsigned)n) continue;
      const int li = ld(&lab[i]), lj = ld(&lab[j]);
      if (li < lj) {
        atomicMin(&lab[j], li);
        ch = true;
      } else if (lj < li) {
        atomicMin(&lab[i], lj);
        ch = true;
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
      const int l = ld(&lab[i]), ll = ld(&lab[l]);
      if (ll < l) {
        atomicMin(&lab[i], ll);
        ch = true;
      }
    }
    if (ch) s_changed = 1;
    __syncthreads();
    if (!s_changed) break;  // uniform: every thread reads the flag after the barrier, and it is reset only after the next one
    __syncthreads();
  }
  __syncthreads();
  // ---- per-atom outputs, fragment sizes, over-valent atoms ------------------------------------------------------------------
  for (int i = tid; i < n; i += 256) {
    const int l = ld(&lab[i]), v2 = ld(&val[i]), t = atom_type[n0 + i];
    component[n0 + i] = l;
    if (small) valence2[n0 + i] = v2;
    atomicAdd(&cnt[l], 1);
    if (l == i) atomicAdd(&s_ncomp, 1);
    const int permitted = (unsigned)t < (unsigned)num_element ? max_valence[t] : 0;
    if (v2 / 2 > permitted) atomicAdd(&s_over, 1);
  }
  // ---- shortest distance over all pairs i < j -------------------------------------------------------------------------------
  {
    unsigned best = 0x7f800000u;  // the 256 threads as 16 x 16: rows i, i + 16, ... against columns j > i
    for (int i = tid >> 4; i < n; i += 16)
      for (int j = i + 1 + (tid & 15); j < n; j += 16) best = min(best, __float_as_uint(dist3(pos, i, j)));
    if (best != 0x7f800000u) atomicMin(&s_dmin, best);
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256)
    if (ld(&lab[i]) == i) atomicMax(&s_best, ((unsigned long long)(unsigned)ld(&cnt[i]) << 32) | (unsigned)(0x7fffffff - i));
  __syncthreads();
  if (tid == 0) {
    n_components[m] = s_ncomp;
    largest_size[m] = (int)(s_best >> 32);
    largest_label[m] = n > 0 ? 0x7fffffff - (int)(s_best & 0xffffffffu) : -1;
    n_overvalent[m] = s_over;
    min_dist[m] = __uint_as_float(s_dmin);
    max_bond_len[m] = __uint_as_float(s_bmax);
  }
}

// one workgroup per molecule; the ballot compaction of decode_compact_kernel (mdx_decode.hip), in place: a kept element moves to
// a position at or below its own, chunks are walked in order and every chunk is read into registers before it is written
__global__ __launch_bounds__(256) void mol_keep_component_kernel(
    const int* __restrict__ node_ptr, const int* __restrict__ he_ptr, const int* __restrict__ select,
    const int* __restrict__ label, const int* __restrict__ component, int* __restrict__ node_new, int* atom_type, float* atom_prob,
    float* atom_pos, int* n_atoms, int* bond_type, float* bond_prob, int* bond_i, int* bond_j, int* n_bonds) {
  __shared__ int wave_cnt[4];
  __shared__ int base;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (select[m] == 0) return;
  const int n0 = node_ptr[m], h0 = he_ptr[m], n = n_atoms[m], nb = n_bonds[m], want = label[m];
  if (tid == 0) base = 0;
  __syncthreads();
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int v = c0 + tid;
    const bool keep = v < n && want >= 0 && component[n0 + v] == want;
    int t = 0;
    float pr = 0.f, x = 0.f, y = 0.f, z = 0.f;
    if (keep) {
      t = atom_type[n0 + v];
      pr = atom_prob[n0 + v];
      x = atom_pos[3 * (size_t)(n0 + v) + 0];
      y = atom_pos[3 * (size_t)(n0 + v) + 1];
      z = atom_pos[3 * (size_t)(n0 + v) + 2];
    }
    const unsigned long long mask = __ballot(keep);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave] = __popcll(mask);
    __syncthreads();  // also: every read of this chunk is done
    int off = base;
    for (int w = 0; w < wave; ++w) off += wave_cnt[w];
    if (v < n) node_new[n0 + v] = keep ? off + before : -1;
    if (keep) {
      const size_t o = (size_t)n0 + off + before;
      atom_type[o] = t;
      atom_prob[o] = pr;
      atom_pos[3 * o + 0] = x;
      atom_pos[3 * o + 1] = y;
      atom_pos[3 * o + 2] = z;
    }
    __syncthreads();
    if (tid == 0) base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    __syncthreads();
  }
  if (tid == 0) {
    n_atoms[m] = base;
    base = 0;
  }
  __syncthreads();  // node_new of this molecule is complete (written by this workgroup) and visible
  for (int c0 = 0; c0 < nb; c0 += 256) {
    const int h = c0 + tid;
    bool keep = false;
    int ni = 0, nj = 0, t = 0;
    float pr = 0.f;
    if (h < nb) {
      const int i = bond_i[h0 + h], j = bond_j[h0 + h];
      if ((unsigned)i < (unsigned)n && (unsigned)j < (unsigned)n) {
        ni = node_new[n0 + i];
        nj = node_new[n0 + j];
        keep = ni >= 0 && nj >= 0;
      }
      t = bond_type[h0 + h];
      pr = bond_prob[h0 + h];
    }
    const unsigned long long mask = __ballot(keep);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave] = __popcll(mask);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wave_cnt[w];
    if (keep) {
      const int o = h0 + off + before;
      bond_type[o] = t;
      bond_prob[o] = pr;
      bond_i[o] = ni;
      bond_j[o] = nj;
    }
    __syncthreads();
    if (tid == 0) base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    __syncthreads();
  }
  if (tid == 0) n_bonds[m] = base;
}

}  // namespace

void launch_mol_check(const MolCheckArgs& a, hipStream_t s) {
  if (a.B > 0)
    hipLaunchKernelGGL(mol_check_kernel, dim3(a.B), dim3(256), 0, s, a.node_ptr, a.he_ptr, a.atom_type, a.atom_pos, a.n_atoms,
                       a.bond_type, a.bond_index, a.bond_index + a.Eh, a.n_bonds, a.max_valence, a.num_element, a.num_bond_types,
                       a.scratch, a.scratch + a.N, a.component, a.valence2, a.n_components, a.largest_size, a.largest_label,
                       a.n_overvalent, a.min_dist, a.max_bond_len);
}

void launch_mol_keep_component(const MolKeepArgs& a, hipStream_t s) {
  if (a.B > 0)
    hipLaunchKernelGGL(mol_keep_component_kernel, dim3(a.B), dim3(256), 0, s, a.node_ptr, a.he_ptr, a.select, a.label,
                       a.component, a.scratch, a.atom_type, a.atom_prob, a.atom_pos, a.n_atoms, a.bond_type, a.bond_prob,
                       a.bond_index, a.bond_index + a.Eh, a.n_bonds);
}
