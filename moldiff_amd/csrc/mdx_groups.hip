// Substructure matching on decoded molecules on the device (mdx_mol_groups): how often, and at which atoms, each pattern of a small
// set occurs in each molecule -- the primitive behind the reference's `groups_counts` (utils/evaluation.py:86-94), the donor / acceptor
// counts of `count_prop`, its PAINS filter and the SMARTS counts of Local3D.get_counts, without RDKit.  The pattern language and every
// output are DEFINED in include/moldiff_hip.h; it is this project's own, NOT SMARTS.  moldiff_amd/groups.py restates the function in
// plain Python and the GPU tests compare every output exactly.
//
// One workgroup of 256 threads (4 waves) per molecule over the compact arrays of mdx_mol.h; a molecule has at most 256 atoms
// and 512 bonds (the caps of mdx_mol_rings), so it is staged ONCE in LDS -- neighbour lists of 16-bit entries (neighbour, bond type,
// ring class of the bond), one attribute word per atom (class, degree, implicit hydrogens, ring class, aromatic flag) -- with the
// translated pattern table beside it, about 13 KB in all: the 8 workgroups a CU's 32 waves allow take 104 of its 160 KB, so occupancy
// is bounded by waves.  The patterns are looped over inside.
// Thread a owns start atom a: it runs an iterative depth-first search for the embeddings that map pattern atom 0 to a.  Pattern
// atoms are ordered so that atom k > 0 has a bond to an earlier atom; the earliest such atom is its parent, and the candidates for k
// are the neighbours of the parent's image.  The stack lives in three 64-bit registers addressed by shifts -- the 8 images as bytes,
// the 8 neighbour-list cursors as 16-bit fields -- because a dynamically indexed register array would go to scratch.  "Already used"
// is a byte comparison against the images; a pattern bond that is not a parent bond is closed by scanning the neighbour list of one
// end for the other.  `steps` counts the candidates by a formula that no traversal order enters (header) and is what max_steps is
// charged in: a thread whose count exceeds it stops, and the pattern is flagged for the molecule.
// Per pattern the sums go through wave reductions and one LDS combine; atom_hit is the owning thread's own word.  All outputs are
// written with plain stores by the workgroup that owns the molecule: no atomics on global memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/moldiff_hip.h"
#include "mdx_groups_args.h"
#include "mdx_mol.h"

namespace {

typedef unsigned long long u64;

constexpr int GP_WAVES = 4;
constexpr int GP_CHUNK = 448;  // table words carried by one launch of the upload kernel, as kernel arguments

struct GpArgs {
  MolArrays mol;
  const int *atom_ring_min, *bond_ring_min, *ring_status;  // all three or none
  const unsigned* table;                                   // GP_WORDS * (1 + P) words (mdx_groups_args.h)
  int num_element, num_bond_types, P, max_steps;
  int *n_embed, *n_anchor, *steps, *pat_status, *status, *atom_hit;
};

struct GpShared {
  unsigned table[GP_TABLE_WORDS];
  unsigned bond[MOL_BONDS];               // the bond word of mdx_mol.h, payload = type | ring class << 5: the high byte of an adj entry
  unsigned attr[MOL_ATOMS];               // class | min(deg, 7) << 5 | min(h, 4) << 8 | ring class << 11 | aromatic << 14 | class known << 15
  int off[MOL_ATOMS + 1], cur[MOL_ATOMS], val2[MOL_ATOMS];
  int red[2][GP_WAVES][4], wave_total[GP_WAVES];
  unsigned short adj[2 * MOL_BONDS];      // neighbour | type << 8 | ring class << 13; type 0 = outside 1 .. num_bond_types
};

struct GpChunkArgs {
  unsigned w[GP_CHUNK];
};

// the validated table travels as kernel arguments: the caller's host array is free as soon as the launch call returns
__global__ __launch_bounds__(256) void groups_table_kernel(const GpChunkArgs c, unsigned* dst, int count) {
  for (int k = threadIdx.x; k < count; k += 256) dst[k] = c.w[k];
}

__device__ inline unsigned ring_class(int r) { return r <= 0 ? 0u : (unsigned)(min(max(r, 3), 8) - 2); }

// status and zeros for a molecule that is not measured; its atom_hit slots only when they are inside the array
__device__ inline void write_unmeasured(const GpArgs& A, int m, int status, const MolView& v) {
  const int tid = threadIdx.x;
  if (tid == 0) A.status[m] = status;
  for (int p = tid; p < A.P; p += 256) {
    const size_t o = (size_t)m * A.P + p;
    A.n_embed[o] = 0, A.n_anchor[o] = 0, A.steps[o] = 0, A.pat_status[o] = 0;
  }
  if (v.outside) return;
  for (int a = tid; a < v.n; a += 256) A.atom_hit[v.n0 + a] = 0;
}

// aw: the pattern atom's word [9 + k], em: its elem_mask
__device__ inline bool atom_ok(unsigned attr, unsigned em, unsigned aw) {
  const unsigned cls = attr & 31u, dc = (attr >> 5) & 7u, hc = (attr >> 8) & 7u, rc = (attr >> 11) & 7u, ar = (attr >> 14) & 1u;
  const unsigned arom = (aw >> 20) & 3u;
  const unsigned bits = (attr >> 15) & (em >> cls) & (aw >> dc) & (aw >> (8u + hc)) & (aw >> (13u + rc)) & 1u;
  return bits != 0u && (arom == 0u || arom == 2u - ar);
}

// bw: type_mask | rsize_mask << 17
__device__ inline bool bond_ok(unsigned ent, unsigned bw) {
  const unsigned t = (ent >> 8) & 31u, rc = (ent >> 13) & 7u;
  return ((bw >> t) & (bw >> (17u + rc)) & 1u) != 0u;  // type 0 meets bit 0 of a type_mask, which is never set
}

// whether byte v is among the low d bytes of img, 1 <= d <= 7
__device__ inline bool used(u64 img, int d, unsigned v) {
  const u64 keep = (1ull << (8 * d)) - 1ull;
  const u64 y = (img ^ (0x0101010101010101ull * v)) | ~keep;  // a zero byte <=> an image equal to v
  return ((y - 0x0101010101010101ull) & ~y & 0x8080808080808080ull) != 0ull;
}

__global__ __launch_bounds__(256) void mol_groups_kernel(const GpArgs A) {
  __shared__ GpShared s;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const MolView v = mol_view(A.mol, m);
  const long long n0 = v.n0, h0 = v.h0;
  const int n = v.n, nb = v.nb;
  if (const int unmeasured = mol_guard(v); unmeasured != MOL_MEASURE) {  // uniform
    write_unmeasured(A, m, unmeasured, v);
    return;
  }
  if (A.ring_status && A.ring_status[m] != 0) {  // uniform
    write_unmeasured(A, m, 2, v);
    return;
  }
  const int *atype = A.mol.atom_type + n0, *bt = A.mol.bond_type + h0;
  const int nbt = A.num_bond_types;

  // ---- the molecule and the table into LDS
  for (int k = tid; k < GP_WORDS * (1 + A.P); k += 256) s.table[k] = A.table[k];
  s.val2[tid] = 0, s.attr[tid] = 0u;
  {
    const int deg = mol_stage_bonds(A.mol, h0, n, nb, s.bond, s.off, s.cur, s.wave_total, [&](int e, int i, int j) {
      int t = bt[e];
      t = t >= 1 && t <= nbt ? t : 0;
      const unsigned rc = A.bond_ring_min ? ring_class(A.bond_ring_min[h0 + e]) : 0u;
      const int w = t == 0 ? 0 : t == nbt ? 3 : 2 * t;  // mdx_mol_check's valence2
      atomicAdd(&s.val2[i], w);
      atomicAdd(&s.val2[j], w);
      if (t == nbt) atomicOr(&s.attr[i], 1u << 14), atomicOr(&s.attr[j], 1u << 14);
      return (unsigned)t | rc << 5;
    });
    if (tid < n) {
      const int cls = atype[tid];
      const bool known = (unsigned)cls < (unsigned)A.num_element;
      const int h = known ? max(0, (int)s.table[cls] - (s.val2[tid] + 1) / 2) : 0;
      const unsigned rc = A.atom_ring_min ? ring_class(A.atom_ring_min[n0 + tid]) : 0u;
      s.attr[tid] = (s.attr[tid] & (1u << 14)) | (known ? (unsigned)cls : 0u) | (unsigned)min(deg, 7) << 5 | (unsigned)min(h, 4) << 8 |
                    rc << 11 | (known ? 1u << 15 : 0u);
    }
  }
  mol_stage_rows(nb, s.bond, s.cur, s.adj, [](unsigned other, int, unsigned bd) { return (unsigned short)(other | mol_bond_payload(bd) << 8); });

  // ---- the patterns: thread a searches the embeddings that send pattern atom 0 to atom a
  unsigned hit = 0u;
  const int a = tid;
  for (int p = 0; p < A.P; ++p) {
    const unsigned* T = s.table + GP_WORDS * (1 + p);
    const int na = (int)T[0];
    int steps = 0, embed = 0;
    bool over = false;
    if (a < n) {
      steps = 1;
      if (atom_ok(s.attr[a], T[1], T[9])) {
        if (na == 1) {
          embed = 1;
        } else {
          u64 img = (u64)a, c0 = 0ull, c1 = 0ull;  // images: byte k; cursors: 16 bits each, atoms 0 .. 3 in c0 and 4 .. 7 in c1
          int d = 1;                              // the pattern atom to place next
          {
            const int lo = s.off[a], hi = s.off[a + 1];  // atom 1's parent is atom 0
            c0 = (u64)lo << 16;
            steps += hi - lo;
            over = steps > A.max_steps;
          }
          // every round either advances a cursor or steps back; `steps` bounds the cursor advances, so the loop ends
          while (!over) {
            const unsigned aw = T[9 + d];
            const int pa = (int)((img >> (8 * ((aw >> 22) & 7u))) & 0xffull);
            const int sh = 16 * (d & 3);
            const int c = (int)(((d < 4 ? c0 : c1) >> sh) & 0xffffull);
            if (c >= s.off[pa + 1]) {
              if (--d == 0) break;
              continue;
            }
            if (d < 4) c0 += 1ull << sh; else c1 += 1ull << sh;
            const unsigned ent = s.adj[c], v = ent & 0xffu;
            bool ok = bond_ok(ent, T[16 + d]) && !used(img, d, v) && atom_ok(s.attr[v], T[1 + d], aw);
            if (ok) {
              const int cf = (aw >> 25) & 7u, cc = (aw >> 28) & 7u;
              for (int q = 0; q < cc && ok; ++q) {
                const unsigned cw = T[24 + cf + q];
                const unsigned want = (unsigned)((img >> (8 * (cw & 7u))) & 0xffull);
                const unsigned bw = ((cw >> 10) & 0x1ffffu) | ((cw >> 3) & 0x7fu) << 17;
                ok = false;
                for (int x = s.off[v], x1 = s.off[v + 1]; x < x1; ++x) {
                  const unsigned e2 = s.adj[x];
                  if ((e2 & 0xffu) == want) {
                    ok = bond_ok(e2, bw);
                    break;
                  }
                }
              }
            }
            if (!ok) continue;
            img = (img & ~(0xffull << (8 * d))) | (u64)v << (8 * d);
            if (d == na - 1) {
              ++embed;
              continue;
            }
            ++d;
            {
              const int np = (int)((img >> (8 * ((T[9 + d] >> 22) & 7u))) & 0xffull);
              const int lo = s.off[np], hi = s.off[np + 1], sh2 = 16 * (d & 3);
              if (d < 4) c0 = (c0 & ~(0xffffull << sh2)) | (u64)lo << sh2; else c1 = (c1 & ~(0xffffull << sh2)) | (u64)lo << sh2;
              steps += hi - lo;
              over = steps > A.max_steps;
            }
          }
        }
      }
    }
    const int e_sum = wave_sum(embed), a_sum = wave_sum(embed > 0 ? 1 : 0), s_sum = wave_sum(steps);
    const bool any_over = __ballot(over) != 0ull;
    int* red = s.red[p & 1][wave];
    if (lane == 0) red[0] = e_sum, red[1] = a_sum, red[2] = s_sum, red[3] = any_over;
    __syncthreads();  // the other half of red[] was read before this barrier of the previous pattern: one barrier per pattern
    int tot[4] = {0, 0, 0, 0};
    for (int w = 0; w < GP_WAVES; ++w)
      for (int k = 0; k < 4; ++k) tot[k] += s.red[p & 1][w][k];
    const bool flagged = tot[3] != 0;
    if (!flagged && embed > 0) hit |= 1u << p;
    if (tid == 0) {
      const size_t o = (size_t)m * A.P + p;
      A.n_embed[o] = flagged ? 0 : tot[0], A.n_anchor[o] = flagged ? 0 : tot[1], A.steps[o] = flagged ? 0 : tot[2];
      A.pat_status[o] = flagged ? 3 : 0;
    }
  }
  if (a < n) A.atom_hit[n0 + a] = (int)hit;
  if (tid == 0) A.status[m] = 0;
}

}  // namespace

extern "C" size_t mdx_mol_groups_ws_bytes(int32_t P) { return groups_ws_bytes(P); }

extern "C" int mdx_mol_groups(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                              const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index,
                              int64_t Eh_stride, const int32_t* select, int32_t num_element, int32_t num_bond_types,
                              const int32_t* normal_valence, const int32_t* patterns, int32_t P, int32_t max_steps,
                              const int32_t* atom_ring_min, const int32_t* bond_ring_min, const int32_t* ring_status, int32_t* n_embed,
                              int32_t* n_anchor, int32_t* steps, int32_t* pat_status, int32_t* status, int32_t* atom_hit, void* ws,
                              size_t ws_bytes, void* stream) {
  GpArgs a{};
  if (const char* why = mol_arrays_fill(&a.mol, B, atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type, N_cap, bond_type, bond_index, Eh_stride, select))
    return mdx_set_error(MDX_ERR_ARG, why);
  if (!normal_valence || !patterns || !n_embed || !n_anchor || !steps || !pat_status || !status || !atom_hit || !ws)
    return mdx_set_error(MDX_ERR_ARG, "null argument");
  if (max_steps < 1 || max_steps > GP_MAX_STEPS) return mdx_set_error(MDX_ERR_ARG, "max_steps must lie in 1 .. 2^20");
  const int given = (atom_ring_min != nullptr) + (bond_ring_min != nullptr) + (ring_status != nullptr);
  if (given != 0 && given != 3) return mdx_set_error(MDX_ERR_ARG, "atom_ring_min, bond_ring_min and ring_status: all three or none");
  uint32_t table[GP_TABLE_WORDS];
  bool needs_rings = false;
  const char* why = "";
  if (groups_prepare(table, normal_valence, patterns, P, num_element, num_bond_types, &needs_rings, &why) != GP_PREP_OK)
    return mdx_set_error(MDX_ERR_ARG, why);
  if (needs_rings && given == 0) return mdx_set_error(MDX_ERR_ARG, "a pattern carries a ring constraint and there is no ring data");
  const int words = GP_WORDS * (1 + P);
  if (((uintptr_t)ws & 3u) != 0 || ws_bytes < sizeof(uint32_t) * (size_t)words)
    return mdx_set_error(MDX_ERR_ARG, "workspace misaligned or smaller than mdx_mol_groups_ws_bytes");
  if (B == 0) return MDX_OK;
  for (int first = 0; first < words; first += GP_CHUNK) {
    GpChunkArgs c;
    const int count = words - first < GP_CHUNK ? words - first : GP_CHUNK;
    for (int k = 0; k < GP_CHUNK; ++k) c.w[k] = k < count ? table[first + k] : 0u;
    hipLaunchKernelGGL(groups_table_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, c, (unsigned*)ws + first, count);
  }
  a.atom_ring_min = atom_ring_min, a.bond_ring_min = bond_ring_min, a.ring_status = ring_status;
  a.table = (const unsigned*)ws;
  a.num_element = num_element, a.num_bond_types = num_bond_types, a.P = P, a.max_steps = max_steps;
  a.n_embed = n_embed, a.n_anchor = n_anchor, a.steps = steps, a.pat_status = pat_status, a.status = status, a.atom_hit = atom_hit;
  return mol_launch(mol_groups_kernel, "mol_groups_kernel", B, stream, a);
}
