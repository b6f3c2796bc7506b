// Kekulé assignment of the aromatic bonds of decoded molecules on the device (mdx_mol_kekulize): which aromatic bonds (the last bond
// type) become double bonds, which atoms take a positive charge or a hydrogen, and whether the aromatic system has a Kekulé structure
// at all -- the pure graph part of what the reference leaves to RDKit's sanitisation and to fix_valence / fix_aromatic
// (utils/reconstruct.py:245-271, :295-387).  It is THIS PROJECT'S OWN MODEL of that step, unverified against RDKit; the rule and every
// output are DEFINED in include/moldiff_hip.h, moldiff_amd/kekule.py restates the function in plain Python and the GPU tests compare
// every output exactly.
//
// The rule in short.  Chemistry is data: normal valence V, charged valence Vc (0 = none) and a flexible bit per atom class.  Per atom
// sigma = the orders of its valid non-aromatic bonds + the number of its aromatic bonds, adeg = the number of its aromatic bonds.  An
// atom with adeg >= 1 has a role: NOT (adeg > 3, or no room: V - sigma < 1 and Vc - sigma < 1), MUST (V - sigma >= 1, not flexible),
// MAY (V - sigma >= 1 and flexible -- it takes a hydrogen instead -- or V - sigma < 1 and Vc - sigma >= 1 -- it takes a charge if
// matched).  Every connected component of the aromatic bonds is searched on its own for a matching on aromatic bonds between atoms
// that are not NOT which covers every MUST atom.  The structure reported is the FIRST one this search finds, and the search order is
// part of the definition: atoms in ascending index; one that is NOT or already matched is skipped; the others try "stay unmatched"
// (MAY only), then every aromatic neighbour of higher index that is not NOT and not yet matched, ascending; with no option left the
// search undoes the previous deciding atom's choice and tries that atom's next option.  `steps` counts the options tried.
//
// One workgroup of 256 threads (4 waves) per molecule over the compact arrays of mdx_mol.h; a molecule has at most 256 atoms and 512
// bonds (the caps of mdx_mol_rings) and is staged ONCE in LDS, about 8 KB.  The components are labelled in LDS by their smallest atom
// (minimum over the aromatic bonds + pointer jumping, until nothing changes); thread a counts the atoms before it in its component
// (its rank: the search order) and in the components before (where the component's table starts).  A component has at most 64 atoms,
// so that ONE THREAD -- the one of its smallest atom -- searches it with the whole state in registers: the matched set and the set
// of deciding atoms are one 64-bit word each over the ranks, the choice stack is 2 bits per atom (stay, neighbour 0 .. 2: an atom with
// more than three aromatic bonds is NOT) in two 64-bit words addressed by shifts.  A runtime-indexed register array would go to
// scratch; there is none, and no recursion.  Per rank one LDS word holds the three candidate neighbours (ranks, ascending) and the
// role.  Every search is bounded by max_steps.  All outputs are written with plain stores by the workgroup that owns the molecule: no
// atomics on global memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/moldiff_hip.h"
#include "mdx_kekule_args.h"
#include "mdx_mol.h"

namespace {

typedef unsigned long long u64;

constexpr int KK_COMPONENT = 64;
constexpr unsigned KK_NONE = 0xffu;                       // no neighbour in this slot
constexpr unsigned short KK_FREE = 0xffff;                // partner of an unmatched atom
enum { ROLE_NONE = 0, ROLE_NOT = 1, ROLE_MUST = 2, ROLE_MAY = 3 };
enum { COMP_SOLVED = 0, COMP_FAILED = 1, COMP_OVER = 2 };
// the columns of mol_stats: MDX_KEKULE_* of include/moldiff_hip.h
enum { K_STATUS, K_AROM_ATOMS, K_AROM_BONDS, K_COMPONENTS, K_FAILED, K_OVER, K_DOUBLE, K_CHARGED, K_HYDROGENS, K_OVERVALENT, K_STEPS };
static_assert(K_STEPS + 1 == KK_STATS && KK_STATS == MDX_KEKULE_STATS, "the columns of mol_stats");

struct KkArgs {
  MolArrays mol;
  KekuleTable tab;
  int num_element, num_bond_types, max_steps;
  int *kek_order, *val, *charge, *kek_h, *atom_flag, *stats;
};

struct KkShared {
  unsigned bond[MOL_BONDS];        // the bond word of mdx_mol.h, payload = type (0: outside 1 .. num_bond_types)
  unsigned nbrw[MOL_ATOMS];        // by place in `list`: the ranks of the candidate neighbours, ascending, bytes 0 .. 2 (0xff: none) | role << 24
  unsigned cand[MOL_ATOMS];        // by atom: the candidate neighbours (atoms) as they arrive, bytes 0 .. 2
  int sigma[MOL_ATOMS], adeg[MOL_ATOMS], label[MOL_ATOMS], ncand[MOL_ATOMS], place[MOL_ATOMS], csteps[MOL_ATOMS];
  int red[KK_STATS], changed, too_big;
  unsigned short partner[MOL_ATOMS];
  unsigned short vtab[KK_MAX_ELEMENTS];
  unsigned char list[MOL_ATOMS];   // the aromatic atoms sorted by (component, atom)
  unsigned char role[MOL_ATOMS], rank[MOL_ATOMS], cstat[MOL_ATOMS];
};

// status and zeros for a molecule that is not measured; its per-atom and per-bond slots only when they are inside the arrays
__device__ inline void write_unmeasured(const KkArgs& A, int m, int status, const MolView& v) {
  const int tid = threadIdx.x;
  if (tid < KK_STATS) A.stats[(size_t)m * KK_STATS + tid] = tid == K_STATUS ? status : 0;
  if (v.outside) return;
  for (int a = tid; a < v.n; a += 256) A.val[v.n0 + a] = 0, A.charge[v.n0 + a] = 0, A.kek_h[v.n0 + a] = 0, A.atom_flag[v.n0 + a] = 0;
  for (int e = tid; e < v.nb; e += 256) A.kek_order[v.h0 + e] = 0;
}

__device__ inline unsigned get2(u64 lo, u64 hi, int r) { return (unsigned)(((r < 32 ? lo : hi) >> (2 * (r & 31))) & 3ull); }

__device__ inline void set2(u64& lo, u64& hi, int r, unsigned c) {
  const int sh = 2 * (r & 31);
  const u64 keep = ~(3ull << sh), put = (u64)c << sh;
  if (r < 32) lo = (lo & keep) | put; else hi = (hi & keep) | put;
}

__global__ __launch_bounds__(256) void mol_kekulize_kernel(const KkArgs A) {
  __shared__ KkShared s;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const MolView v = mol_view(A.mol, m);
  const long long n0 = v.n0, h0 = v.h0;
  const int n = v.n, nb = v.nb;
  if (const int unmeasured = mol_guard(v); unmeasured != MOL_MEASURE) {  // uniform
    write_unmeasured(A, m, unmeasured, v);
    return;
  }
  const int *atype = A.mol.atom_type + n0, *bi = A.mol.bond_i + h0, *bj = A.mol.bond_j + h0, *bt = A.mol.bond_type + h0;
  const int nbt = A.num_bond_types;

  // ---- the molecule into LDS: bonds, sigma, adeg
  s.sigma[tid] = 0, s.adeg[tid] = 0, s.ncand[tid] = 0, s.cand[tid] = 0u, s.label[tid] = tid, s.csteps[tid] = 0;
  s.partner[tid] = KK_FREE, s.role[tid] = ROLE_NONE, s.cstat[tid] = COMP_SOLVED, s.rank[tid] = 0, s.place[tid] = 0;
  if (tid < KK_MAX_ELEMENTS) s.vtab[tid] = A.tab.valence[tid];
  if (tid < KK_STATS) s.red[tid] = 0;
  if (tid == 0) s.too_big = 0;
  __syncthreads();
  for (int e = tid; e < nb; e += 256) {
    const int i = bi[e], j = bj[e];
    if (!mol_bond_ok(i, j, n)) {
      s.bond[e] = 0u;
      continue;
    }
    int t = bt[e];
    t = t >= 1 && t <= nbt ? t : 0;
    s.bond[e] = mol_bond_word(i, j, (unsigned)t);
    if (t == 0) continue;
    const int w = t == nbt ? 1 : t;
    atomicAdd(&s.sigma[i], w);
    atomicAdd(&s.sigma[j], w);
    if (t == nbt) atomicAdd(&s.adeg[i], 1), atomicAdd(&s.adeg[j], 1);
  }
  __syncthreads();

  // ---- roles
  const int my_adeg = s.adeg[tid];  // 0 past the molecule
  if (tid < n && my_adeg > 0) {
    const int cls = atype[tid];
    const bool known = (unsigned)cls < (unsigned)A.num_element;
    const int V = known ? s.vtab[cls] & 0xff : 0, Vc = known ? s.vtab[cls] >> 8 : 0;
    const bool flexible = known && ((A.tab.flexible >> cls) & 1u);
    const int sg = s.sigma[tid];
    int role = ROLE_NOT;
    if (my_adeg <= 3) {
      if (V - sg >= 1) role = flexible ? ROLE_MAY : ROLE_MUST;
      else if (Vc - sg >= 1) role = ROLE_MAY;
    }
    s.role[tid] = (unsigned char)role;
  }

  // ---- the components of the aromatic bonds, each labelled by its smallest atom.  A round lowers every label that is not yet the
  // smallest of its component or ends the loop, and labels only fall: at most 255 rounds.
  for (int round = 0; round < MOL_ATOMS; ++round) {
    __syncthreads();  // the previous round's `changed` has been read (and, first, the roles are visible)
    if (tid == 0) s.changed = 0;
    __syncthreads();
    for (int e = tid; e < nb; e += 256) {
      const unsigned bd = s.bond[e];
      if ((int)mol_bond_payload(bd) != nbt || !bd) continue;
      const int i = mol_bond_i(bd), j = mol_bond_j(bd);
      const int li = ((volatile int*)s.label)[i], lj = ((volatile int*)s.label)[j];
      if (li == lj) continue;
      atomicMin(&s.label[li < lj ? j : i], min(li, lj));
      s.changed = 1;
    }
    __syncthreads();
    {  // pointer jumping: a label is an atom of the same component, and so is that atom's label
      const int l = ((volatile int*)s.label)[tid], ll = ((volatile int*)s.label)[l];
      if (ll < l) ((volatile int*)s.label)[tid] = ll, s.changed = 1;
    }
    __syncthreads();
    if (!s.changed) break;  // uniform
  }

  // ---- the candidate neighbours of every atom that may be matched: the aromatic neighbours of higher index that are not NOT
  for (int e = tid; e < nb; e += 256) {
    const unsigned bd = s.bond[e];
    if ((int)mol_bond_payload(bd) != nbt || !bd) continue;
    const unsigned i = mol_bond_i(bd), j = mol_bond_j(bd), lo = min(i, j), hi = max(i, j);
    if (s.role[lo] == ROLE_NOT || s.role[hi] == ROLE_NOT) continue;
    const int slot = atomicAdd(&s.ncand[lo], 1);
    if (slot < 3) atomicOr(&s.cand[lo], hi << (8 * slot));  // adeg <= 3 here: a fourth arrives only with the precondition violated
  }
  // ---- rank in the component (the search order), the component's size, the place in the sorted list
  const int my_label = s.label[tid];
  int my_size = 0;
  if (tid < n && my_adeg > 0) {
    int rank = 0, before = 0;
    for (int b = 0; b < n; ++b) {
      if (s.adeg[b] == 0) continue;
      const int lb = s.label[b];
      my_size += lb == my_label;
      rank += lb == my_label && b < tid;
      before += lb < my_label;
    }
    if (my_size > KK_COMPONENT) s.too_big = 1;
    s.rank[tid] = (unsigned char)min(rank, 255);
    s.place[tid] = before + rank;  // < n
    s.list[before + rank] = (unsigned char)tid;
  }
  __syncthreads();
  if (s.too_big) {  // uniform
    write_unmeasured(A, m, 1, v);
    return;
  }
  if (tid < n && my_adeg > 0) {
    unsigned r[3];
    const unsigned c = s.cand[tid];
    const int k = min(s.ncand[tid], 3);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const unsigned b = (c >> (8 * q)) & 0xffu;
      r[q] = q < k && s.label[b] == my_label ? (unsigned)s.rank[b] : KK_NONE;  // a rank is below 64
    }
    // ascending; KK_NONE sorts last
    unsigned t;
    if (r[0] > r[1]) t = r[0], r[0] = r[1], r[1] = t;
    if (r[1] > r[2]) t = r[1], r[1] = r[2], r[2] = t;
    if (r[0] > r[1]) t = r[0], r[0] = r[1], r[1] = t;
    s.nbrw[s.place[tid]] = r[0] | r[1] << 8 | r[2] << 16 | (unsigned)s.role[tid] << 24;
  }
  __syncthreads();

  // ---- the search: the thread of a component's smallest atom
  if (tid < n && my_adeg > 0 && my_label == tid) {
    const int base = s.place[tid], count = my_size;  // base + count <= n
    u64 decide = 0ull, may = 0ull;
    for (int r = 0; r < count; ++r) {
      const unsigned role = s.nbrw[base + r] >> 24;
      if (role != ROLE_NOT) decide |= 1ull << r;
      if (role == ROLE_MAY) may |= 1ull << r;
    }
    u64 matched = 0ull, decided = 0ull, clo = 0ull, chi = 0ull;
    int status = COMP_SOLVED, steps = 0, from = 0;
    // every round of the inner loop tries an option (a step: at most max_steps of them) or takes a deciding atom off the stack
    for (;;) {
      const u64 open = decide & ~matched & (from >= 64 ? 0ull : ~0ull << from);
      if (open == 0ull) break;  // past the last atom: solved
      int r = __ffsll((long long)open) - 1;
      unsigned opt = (may >> r) & 1ull ? 0u : 1u;  // 0: stay unmatched; 1 .. 3: the neighbour in slot opt - 1
      bool placed = false;
      for (;;) {
        const unsigned w = s.nbrw[base + r];
        unsigned nr = 0u;
        for (; opt < 4u; ++opt) {
          if (opt == 0u) break;
          nr = (w >> (8 * (opt - 1u))) & 0xffu;
          if (nr < (unsigned)KK_COMPONENT && !((matched >> nr) & 1ull)) break;
        }
        if (opt < 4u) {
          if (steps == A.max_steps) {
            status = COMP_OVER;
            break;
          }
          ++steps;
          set2(clo, chi, r, opt);
          decided |= 1ull << r;
          if (opt) matched |= 1ull << r | 1ull << nr;
          from = r + 1;
          placed = true;
          break;
        }
        if (decided == 0ull) {
          status = COMP_FAILED;
          break;
        }
        r = 63 - __clzll((long long)decided);
        decided &= ~(1ull << r);
        const unsigned c = get2(clo, chi, r);
        if (c) matched &= ~(1ull << r | 1ull << ((s.nbrw[base + r] >> (8 * (c - 1u))) & 0x3fu));
        opt = c + 1u;
      }
      if (!placed) break;
    }
    s.cstat[tid] = (unsigned char)status;
    s.csteps[tid] = status == COMP_OVER ? 0 : steps;
    if (status == COMP_SOLVED) {
      while (decided != 0ull) {
        const int r = __ffsll((long long)decided) - 1;
        decided &= decided - 1ull;
        const unsigned c = get2(clo, chi, r);
        if (!c) continue;
        const unsigned nr = (s.nbrw[base + r] >> (8 * (c - 1u))) & 0x3fu;
        const unsigned x = s.list[base + r], y = s.list[min(base + (int)nr, MOL_ATOMS - 1)];
        s.partner[x] = (unsigned short)y, s.partner[y] = (unsigned short)x;
      }
    }
  }
  __syncthreads();

  // ---- results
  int red[KK_STATS];
#pragma unroll
  for (int k = 0; k < KK_STATS; ++k) red[k] = 0;
  if (tid < n) {
    const int cls = atype[tid];
    const bool known = (unsigned)cls < (unsigned)A.num_element;
    const int V = known ? s.vtab[cls] & 0xff : 0, Vc = known ? s.vtab[cls] >> 8 : 0;
    const bool root = my_adeg > 0 && my_label == tid;
    const int cstat = my_adeg > 0 ? s.cstat[my_label] : COMP_SOLVED;
    const bool bad = cstat != COMP_SOLVED, matched = s.partner[tid] != KK_FREE;
    const int val = s.sigma[tid] + (matched ? 1 : 0);
    const int charge = !bad && V < val && val <= Vc ? 1 : 0;
    const int h = bad ? 0 : max(0, (charge ? Vc : V) - val);
    const bool over = val > max(V, Vc);
    A.val[n0 + tid] = val, A.charge[n0 + tid] = charge, A.kek_h[n0 + tid] = h;
    A.atom_flag[n0 + tid] = (int)s.role[tid] | (matched ? 4 : 0) | (over ? 8 : 0) | (bad ? 16 : 0);
    red[K_AROM_ATOMS] = my_adeg > 0, red[K_COMPONENTS] = root, red[K_FAILED] = root && cstat == COMP_FAILED;
    red[K_OVER] = root && cstat == COMP_OVER, red[K_DOUBLE] = matched, red[K_CHARGED] = charge, red[K_HYDROGENS] = h;
    red[K_OVERVALENT] = over, red[K_STEPS] = root ? s.csteps[tid] : 0;
  }
  for (int e = tid; e < nb; e += 256) {
    const unsigned bd = s.bond[e];
    const int t = mol_bond_payload(bd);
    int order = 0;
    if (bd && t > 0) {
      const unsigned i = mol_bond_i(bd), j = mol_bond_j(bd);
      if (t < nbt) {
        order = t;
      } else {
        ++red[K_AROM_BONDS];
        if (s.cstat[s.label[i]] == COMP_SOLVED) order = s.partner[i] == j ? 2 : 1;
      }
    }
    A.kek_order[h0 + e] = order;
  }
#pragma unroll
  for (int k = 1; k < KK_STATS; ++k) {
    const int sum = wave_sum(red[k]);
    if (lane == 0 && sum) atomicAdd(&s.red[k], sum);
  }
  __syncthreads();
  if (tid < KK_STATS) A.stats[(size_t)m * KK_STATS + tid] = tid == K_STATUS ? 0 : tid == K_DOUBLE ? s.red[tid] / 2 : s.red[tid];
}

}  // namespace

extern "C" int mdx_mol_kekulize(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                                const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index,
                                int64_t Eh_stride, const int32_t* select, int32_t num_element, int32_t num_bond_types,
                                const int32_t* normal_valence, const int32_t* charged_valence, uint32_t flexible, int32_t max_steps,
                                int32_t* kek_order, int32_t* val, int32_t* charge, int32_t* kek_h, int32_t* atom_flag, int32_t* mol_stats,
                                void* stream) {
  KkArgs a{};
  if (const char* why = mol_arrays_fill(&a.mol, B, atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type, N_cap, bond_type, bond_index, Eh_stride, select))
    return mdx_set_error(MDX_ERR_ARG, why);
  if (!normal_valence || !charged_valence || !kek_order || !val || !charge || !kek_h || !atom_flag || !mol_stats)
    return mdx_set_error(MDX_ERR_ARG, "null argument");
  const char* why = "";
  if (kekule_prepare(&a.tab, normal_valence, charged_valence, flexible, num_element, num_bond_types, max_steps, &why) != KK_PREP_OK)
    return mdx_set_error(MDX_ERR_ARG, why);
  a.num_element = num_element, a.num_bond_types = num_bond_types, a.max_steps = max_steps;
  a.kek_order = kek_order, a.val = val, a.charge = charge, a.kek_h = kek_h, a.atom_flag = atom_flag, a.stats = mol_stats;
  return mol_launch(mol_kekulize_kernel, "mol_kekulize_kernel", B, stream, a);
}
