"""Sampling entry point -- the MI355X counterpart of the reference's ``scripts/sample_drug3d.py``.

    python -m moldiff_amd.sample_drug3d --config configs/sample_MolDiff_simple.yml --outdir ./outputs \
        --device cuda:0 [--batch_size N] [--recipe-weights] [--scaffold scaffold.mol] [--accept valence] [--largest_fragment 0.8] [--kekulize] [--canonical] [--stereo] [--conformers] [--frameworks] [--hydrogens] [--relax] [--global3d N]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m moldiff_amd.sample_drug3d ...

Same flags (--config --outdir --device --batch_size), same YAML keys (model.checkpoint, bond_predictor,
sample.{seed,batch_size,num_mols,save_traj_prob,guidance}), same seeding rule (seed + sum(ord(outdir)),
scripts/sample_drug3d.py:47), same batch-size rule ``min(batch_size, 2*remaining)`` (:112) and the same
give-up rule (:106-108).  What differs, deliberately:
  * the hot path runs in the HIP library, and decode/compaction of the predictions runs on the device
    (``FeaturizeMol.decode_batch``) instead of a per-molecule numpy loop over a full D2H copy;
  * RDKit reconstruction (utils/reconstruct.py, CPU chemistry) is out of scope: a molecule counts as
    finished when its decoded bond graph is connected (the reference's test is "no '.' in the SMILES");
    molecules are written as V2000 mol blocks (bond order 4 = aromatic) and collected in ``samples_all.pt``;
  * ``sample.save_traj_prob``: the trajectory is kept compact on the device (class ids, one byte per atom / half-edge and
    frame) and only the drawn molecules' frames are decoded (``traj_mol<id>.sdf``, one mol block per frame); the draw is a
    function of (seed, global molecule id) instead of the position in numpy's global stream, so it does not depend on the
    number of GPUs;
  * with WORLD_SIZE > 1 every rank samples a contiguous slice of each batch's cost-balanced molecule order (noise keyed by
    global molecule id); per batch the last-step predictions travel to rank 0 as tensors (``distributed.gather_pred``:
    one count all_gather + ONE padded gather-to-rank-0 of a flat buffer holding all three) and one 2-element all-reduce carries the loop condition.
``--scaffold PATH`` (config key ``sample.scaffold``), an addition beyond the reference: PATH is a V2000 mol block as this module
writes them; every sampled molecule gets it as its first atoms, held fixed with the bonds among them, and the rest is grown around
it (``moldiff_amd/scaffold.py``).  Sizes are drawn as usual and raised to the scaffold's atom count where they fall below it.
``--accept {connected,valence}`` / ``--largest_fragment FRAC`` (config keys ``sample.accept``, ``sample.largest_fragment``), additions
beyond the reference: with either, acceptance comes from the device-side quality check (``FeaturizeMol.check_batch``) instead of the
Python union-find -- 'connected' is the rule above, 'valence' adds "no atom above its largest permitted valence" (a NECESSARY
condition of the reference's RDKit sanitisation, from a table that is unchecked against RDKit: moldiff_amd/molcheck.py); FRAC in
(0, 1], no default, replaces a disconnected molecule whose largest fragment holds at least FRAC of its atoms by that fragment before
it is judged.  Pool entries then carry n_components / n_overvalent / min_dist / max_bond_len (of the molecule as decoded) and
salvaged, and rank 0 writes ``quality.json`` into the log directory.  Without both options nothing changes.
``--local3d PATTERNS.yml`` (config key ``sample.local3d``; the flag wins), an addition beyond the reference: rank 0 accumulates the bond
length / bond angle / dihedral histograms of the FINISHED molecules of every batch on the device (``moldiff_amd/local3d.py``; with
``--largest_fragment`` a salvaged molecule is its fragment) and writes ``local3d.npz`` beside ``samples_all.pt``; compare two runs with
``python -m moldiff_amd.local3d compare``.  Without the option nothing changes.
``--similarity [REFERENCE.npz]`` (config key ``sample.similarity``: true or a path; the flag wins), an addition beyond the reference:
rank 0 fingerprints the same FINISHED molecules on the device batch by batch (``moldiff_amd/similarity.py``: this project's fingerprint
and key, not RDKit's) and writes ``fingerprints.npz`` and ``similarity.json`` -- uniqueness and diversity, and with a reference
fingerprint file novelty and similarity against it -- beside ``samples_all.pt``.  Without the option nothing changes.
``--rings`` (config key ``sample.rings``; the flag wins), an addition beyond the reference: rank 0 measures the rings and the
composition of the same FINISHED molecules on the device batch by batch (``moldiff_amd/rings.py``: ring sizes of a minimum cycle basis,
not RDKit's SSSR; this project's rotatable-bond rule) and writes ``rings.npz`` (per-molecule arrays) and ``rings.json`` (their summary)
beside ``samples_all.pt``.  Without the option nothing changes.
``--groups [PATTERNS.yml]`` (config key ``sample.groups``: true or a path; the flag wins), an addition beyond the reference: rank 0 counts
the functional groups of the same FINISHED molecules on the device batch by batch (``moldiff_amd/groups.py``: a substructure matcher
with this project's own pattern language, not SMARTS; bare, the default set ``configs/groups_default.yml``) and writes ``groups.npz``
(per-molecule arrays) and ``groups.json`` (their summary) beside ``samples_all.pt``.  Without the option nothing changes.
``--kekulize`` (config key ``sample.kekulize``; the flag wins) and ``--accept kekule``, additions beyond the reference: rank 0 assigns a
Kekulé structure to the aromatic bonds of the decoded molecules on the device batch by batch (``moldiff_amd/kekule.py``: this project's
model of the kekulisation step of RDKit's sanitisation, default tables unverified against RDKit, the first structure in search order and
not a charge-minimal one).  ``--kekulize`` writes ``kekule.npz`` (per-molecule, per-atom and per-bond arrays of the FINISHED molecules),
``kekule.json`` (their summary) and ``samples_kekule.sdf`` (the finished molecules that are kekulizable, bond orders 1 / 2 / 3 and
``M  CHG`` lines) beside ``samples_all.pt``; ``--accept kekule`` is 'valence' and kekulizable.  With either, pool entries carry
``kekulizable`` and ``quality.json`` (written with ``--accept`` / ``--largest_fragment``) gains its count.  Without both nothing changes.
``--canonical`` (config key ``sample.canonical``; the flag wins), an addition beyond the reference: rank 0 labels the FINISHED molecules
canonically on the device batch by batch (``moldiff_amd/canon.py``: this project's own canonical form, not RDKit's canonical ranking) and
writes ``canon.npz`` (per-molecule arrays, ``rank``, ``orbit`` and the canonical arrays) and ``canon.json`` (their summary, with the
EXACT uniqueness by full certificate) beside ``samples_all.pt``.  Together with ``--kekulize`` it also writes ``samples.smi``, one line
``SMILES<TAB>mol_id`` per finished molecule that has a string, and pool entries gain ``smiles`` (this project's own string from the
canonical order and the Kekulé structure of the canonical form; unchecked against RDKit).  ``kekule.npz`` and ``samples_kekule.sdf``
stay what they are, from the molecule as decoded.  ``--canonical_max_nodes`` (``sample.canonical_max_nodes``) is the search budget: a
molecule whose unpruned tree is larger is reported as abandoned (status 2), which is what the nearly complete bond graphs of untrained
weights get.  Without the option nothing changes.
``--stereo`` (config key ``sample.stereo``; the flag wins; it implies ``--canonical``), an addition beyond the reference: rank 0 perceives
the stereo of the FINISHED molecules from their coordinates on the device batch by batch (``moldiff_amd/stereo.py``: this project's own
model, not RDKit's perception and not CIP, unverified against RDKit, blind to allenes, atropisomers and nitrogen inversion) and writes
``stereo.npz`` (per-molecule arrays, the canonical stereo words, ``stereo_rank``, ``atom_tetra``, ``bond_stereo``) and ``stereo.json``
(their summary with the isomeric uniqueness, the share of chiral molecules and of flat centres).  ``--stereo_flat_tol`` /
``--stereo_bond_tol`` (``sample.stereo_flat_tol`` / ``sample.stereo_bond_tol``; 0.1 each) are the two thresholds.  With ``--kekulize`` the
strings of ``samples.smi`` are isomeric ('@', '/'); ``canon.npz`` and ``canon.json`` stay what they are.  Without the option nothing changes.
``--hydrogens`` (config key ``sample.hydrogens``; the flag wins; implies ``--kekulize``), an addition beyond the reference: rank 0 places
the hydrogens of the Kekulé assignment on the FINISHED molecules on the device batch by batch (``moldiff_amd/hydrogens.py``: this
project's own idealised placement, not RDKit's AddHs, unverified against RDKit; rotor torsions by rule, lengths by convention) and writes
``hydrogens.npz`` (counts, flags, positions, shortest contacts), ``hydrogens.json`` (their summary) and ``samples_allatom.sdf`` (the
kekulizable finished molecules as all-atom mol blocks) beside ``samples_all.pt``.  ``--clash_tol`` (``sample.clash_tol``; 1.5 Angstrom: a
convention, untuned) is the contact length below which a pair counts as a clash.  No acceptance rule is added; without the option
nothing changes.
``--relax`` (config key ``sample.relax``; the flag wins; implies ``--hydrogens``), an addition beyond the reference: rank 0 relaxes the
all-atom FINISHED molecules in a UFF-form force field on the device batch by batch (``moldiff_amd/relax.py``: this project's own model
over an unverified parameter table, not RDKit's UFFOptimizeMolecule, unverified against RDKit) and writes ``relax.npz`` (statuses,
energies before and after, relaxed positions), ``relax.json`` (their summary: strain, convergence shares, histograms) and
``samples_relaxed.sdf`` (the kekulizable, relaxed molecules as all-atom mol blocks) beside ``samples_all.pt``.  ``--relax_iters``
(``sample.relax_iters``; 200) and ``--relax_gtol`` (``sample.relax_gtol``; 1e-2 kcal/mol/Angstrom: a convention) bound the minimiser.  No
acceptance rule is added; without the option nothing changes.
``--global3d N`` (config key ``sample.global3d``; the flag wins; implies ``--hydrogens``), an addition beyond the reference's sampling
script: rank 0 generates N conformers of every FINISHED molecule on the device batch by batch (``moldiff_amd/embed.py``: distance
bounds, embedding from random coordinates keyed by ``--global3d_seed`` (``sample.global3d_seed``; 0) and the molecule's id, then the
relaxation of ``--relax`` with its defaults), takes the best RMSD of every conformer against the molecule and writes ``global3d.npz``
(statuses, deviations, conformer coordinates), ``global3d.json`` (their summary) and ``conformers.sdf`` (the conformers that count
as all-atom mol blocks) beside ``samples_all.pt``.  This project's own model, not ETKDG + UFF, unverified against RDKit; stereocentres
are not constrained, so a conformer may be the mirror image and the mirror-image numbers are reported beside the plain ones.  Without
the option nothing changes.
``--frameworks`` (config key ``sample.frameworks``; the flag wins), an addition beyond the reference: rank 0 cuts the FINISHED molecules
into framework, ring systems, linkers and side chains on the device batch by batch (``moldiff_amd/framework.py``: this project's own
definition, not RDKit's MurckoScaffold), keys the pieces with the canonical labelling and writes ``frameworks.npz`` (results and keys)
and ``frameworks.json`` (their summary).  ``--frameworks_exo`` / ``--frameworks_generic`` (``sample.frameworks_exo`` /
``sample.frameworks_generic``) set the mode bits; ``--canonical_max_nodes`` is the search budget of the keys: a piece whose search is
abandoned has no key and is counted in the summary.  Without the option nothing changes.
No pretrained checkpoint ships with the reference (Google-Drive download); ``--recipe-weights`` substitutes the
deterministic synthetic weights used by the tests so the entry point can be exercised end to end.
"""
import argparse
import json
import os
import shutil
import time
from typing import Any, Callable, NamedTuple

import numpy as np
import torch

from . import BondPredictor, MolDiff, _lib
from .distributed import balanced_order, gather_pred, shard_bounds
from .harness import default_config, load_config, placeholder_from_sizes, recipe_state_dict, seed_all
from .harness import GEOM_DRUGS_MEAN_ATOMS, GEOM_DRUGS_STD_ATOMS
from .molpack import ELEMENT_SYMBOL, save_npz, to_host
from .molcheck import accept_rule, fragment_fraction, judge, quality_summary
from .postprocess import FeaturizeMol
from .scaffold import scaffold_for_sizes


class Feature(NamedTuple):
    """One "parts, then files" evaluation of the finished molecules: `run` on every batch's finished molecules gives a results dict,
    `module` joins the parts (``concat``; ``empty`` when there was none) and sums them up (``summary``), and STEM.npz / STEM.json hold
    the two.  `empty` and `summary` stand in where the module's own need arguments; `after` writes any further file from the results."""
    run: Callable
    module: Any
    stem: str
    empty: Callable = None
    summary: Callable = None
    after: Callable = None


def is_connected(n_atoms, bond_index):
    """True when the undirected bond graph over n_atoms has one component (= no '.' in a SMILES)."""
    if n_atoms == 0:
        return False
    parent = list(range(n_atoms))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, j in bond_index.T:
        ri, rj = find(int(i)), find(int(j))
        if ri != rj:
            parent[ri] = rj
    return len({find(i) for i in range(n_atoms)}) == 1


def mol_block(info, name='moldiff_amd'):
    """V2000 mol block from a decode_output dict (one line per directed-pair's first half)."""
    ele, pos = info['element'], info['atom_pos']
    nb = info['bond_index'].shape[1] // 2
    lines = [name, '  moldiff_amd', '', '%3d%3d  0  0  0  0  0  0  0  0999 V2000' % (len(ele), nb)]
    for e, p in zip(ele, pos):
        lines.append('%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0' % (p[0], p[1], p[2], ELEMENT_SYMBOL.get(int(e), 'X')))
    for k in range(nb):
        lines.append('%3d%3d%3d  0' % (info['bond_index'][0, k] + 1, info['bond_index'][1, k] + 1, info['bond_type'][k]))
    lines.append('M  END')
    return '\n'.join(lines) + '\n'


def read_mol_block(text):
    """Inverse of ``mol_block``: a V2000 mol block -> dict(element (n) atomic numbers, atom_pos (n,3) float32, bond_index (2,2b),
    bond_type (2b)) in decode_output's layout (each bond once in file order, then all of them flipped).  Host code; coordinates carry
    the four decimals the block prints.  An element symbol this module does not write raises."""
    lines = text.splitlines()
    counts = next((k for k, ln in enumerate(lines) if ln.rstrip().endswith('V2000')), None)
    if counts is None:
        raise ValueError('not a V2000 mol block (no counts line)')
    na, nb = int(lines[counts][0:3]), int(lines[counts][3:6])
    number = {sym: z for z, sym in ELEMENT_SYMBOL.items()}
    ele, pos = [], []
    for ln in lines[counts + 1:counts + 1 + na]:
        sym = ln[31:34].strip()
        if sym not in number:
            raise ValueError(f'unknown element {sym!r} in mol block (known: {sorted(number)})')
        ele.append(number[sym])
        pos.append([float(ln[0:10]), float(ln[10:20]), float(ln[20:30])])
    bi, bt = [], []
    for ln in lines[counts + 1 + na:counts + 1 + na + nb]:
        bi.append([int(ln[0:3]) - 1, int(ln[3:6]) - 1])
        bt.append(int(ln[6:9]))
    if len(ele) != na or len(bt) != nb:
        raise ValueError('truncated mol block')
    idx = np.asarray(bi, dtype=np.int64).reshape(nb, 2).T
    return {'element': np.asarray(ele, dtype=np.int64), 'atom_pos': np.asarray(pos, dtype=np.float32).reshape(na, 3),
            'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.asarray(bt + bt, dtype=np.int64)}


def build_models(config, device, recipe):
    ckpt_path = config.model.checkpoint
    if os.path.exists(ckpt_path):
        ckpt = torch.load(ckpt_path, map_location='cpu', weights_only=False)
        train_config = ckpt['config']
        model = MolDiff(train_config.model, 8, 6)
        model.load_state_dict(ckpt['model'])
    elif recipe:
        kind = 'MolDiff' if 'bond_predictor' in config else 'MolDiff_simple'
        model = MolDiff(default_config(kind), 8, 6)
        model.load_state_dict(recipe_state_dict(model, 20230807))
        train_config = None
    else:
        raise FileNotFoundError(f'{ckpt_path} not found (the reference distributes checkpoints via Google Drive); '
                                f'pass --recipe-weights to run with synthetic weights')
    model = model.to(device).eval()
    bond_predictor, guidance = None, None
    if 'bond_predictor' in config:
        bp_path = config.bond_predictor
        if os.path.exists(bp_path):
            ck = torch.load(bp_path, map_location='cpu', weights_only=False)
            bond_predictor = BondPredictor(ck['config']['model'], 8, 5)
            bond_predictor.load_state_dict(ck['model'])
        elif recipe:
            bond_predictor = BondPredictor(default_config('bondpred'), 8, 5)
            bond_predictor.load_state_dict(recipe_state_dict(bond_predictor, 20230808))
        else:
            raise FileNotFoundError(bp_path)
        bond_predictor = bond_predictor.to(device).eval()
        # MOLDIFF_GUIDANCE_MATRIX_PATH=split_f16: only the guidance predictor on the split float16 path, the denoiser stays where
        # MOLDIFF_MATRIX_PATH puts it (exact fp32 by default) -- the 'mixed' configuration of DESIGN.md section 3.4
        gpath = os.environ.get('MOLDIFF_GUIDANCE_MATRIX_PATH')
        if gpath:
            bond_predictor.matrix_path = _lib.resolve_matrix_path(gpath)
    if 'guidance' in config.sample:
        guidance = config.sample.guidance
    return model, bond_predictor, guidance


def traj_blocks(featurizer, traj, sel, sizes, device):
    """Trajectories of the molecules `sel` (batch-local indices) as lists of decode_output dicts, one per frame
    (scripts/sample_drug3d.py:157-163).  The frames are cut out of the compact trajectory (class ids, one byte each),
    re-packed as a small batch of their own and decoded on the device frame by frame with ``decode_batch``."""
    node_traj, pos_traj, half_traj = traj
    sizes = np.asarray(sizes, dtype=np.int64)
    node_off = np.concatenate([[0], np.cumsum(sizes)])
    half_off = np.concatenate([[0], np.cumsum(sizes * (sizes - 1) // 2)])
    nidx = torch.as_tensor(np.concatenate([np.arange(node_off[m], node_off[m + 1]) for m in sel]), device=device)
    hidx = torch.as_tensor(np.concatenate([np.arange(half_off[m], half_off[m + 1]) for m in sel]), device=device)
    sub = placeholder_from_sizes(sizes[list(sel)], device)
    graph = _lib.Graph(torch.cat([sub['halfedge_index'], sub['halfedge_index'].flip(0)], dim=1), sub['batch_node'], len(sel))
    nt, pt, ht = node_traj[:, nidx], pos_traj[:, nidx], half_traj[:, hidx]   # still compact
    frames = []
    for t in range(pt.shape[0]):
        frames.append(featurizer.decode_batch([nt[t].dense(), pt[t].contiguous(), ht[t].dense()], sub['batch_node'],
                                              sub['halfedge_index'], sub['batch_halfedge'], len(sel), graph=graph))
    return {m: [frames[t][j] for t in range(len(frames))] for j, m in enumerate(sel)}


def quality_options(accept, largest_fragment, sample_cfg):
    """(rule, FRAC or None, active) from the command line's values (None = not given) and the config's ``sample`` section; a value
    outside what the options admit raises ValueError.  active = either option was given: acceptance then comes from check_batch."""
    if accept is None:
        accept = sample_cfg.get('accept')
    if largest_fragment is None:
        largest_fragment = sample_cfg.get('largest_fragment')
    active = accept is not None or largest_fragment is not None
    if largest_fragment is not None:
        fragment_fraction(largest_fragment)
        largest_fragment = float(largest_fragment)
    return accept_rule('connected' if accept is None else accept), largest_fragment, active


def local3d_option(flag, sample_cfg):
    """path of the pattern file from the command line's value (None or '' = not given) and the config's ``sample`` section, or None:
    the flag wins over ``sample.local3d``"""
    return flag or sample_cfg.get('local3d') or None


def similarity_option(flag, sample_cfg):
    """(active, path of the reference fingerprint file or None) from the command line's value (None = not given, True = given bare)
    and the config's ``sample`` section (``similarity``: true or a path); the flag wins"""
    value = flag if flag is not None else sample_cfg.get('similarity')
    if value is None or value is False or value == '':
        return False, None
    return True, (None if value is True else str(value))


def add_similarity_argument(ap):
    """``--similarity [REFERENCE.npz]`` on a parser of ``build_parser``, whose own option set stays what it was"""
    ap.add_argument('--similarity', nargs='?', const=True, default=None, metavar='REFERENCE.npz',
                    help='fingerprint the finished molecules on the device and write fingerprints.npz and similarity.json (uniqueness, '
                         'diversity; with a reference fingerprint file also novelty and similarity against it; overrides '
                         'sample.similarity)')
    return ap


def rings_option(flag, sample_cfg):
    """whether to measure rings: the command line's flag (None = not given) wins over the config's ``sample.rings``"""
    return bool(flag if flag is not None else sample_cfg.get('rings'))


def add_rings_argument(ap):
    """``--rings`` on a parser of ``build_parser``, whose own option set stays what it was"""
    ap.add_argument('--rings', action='store_true', default=None,
                    help='measure ring sizes, ring atoms, rotatable bonds and the element / bond type counts of the finished molecules '
                         'on the device and write rings.npz and rings.json (overrides sample.rings)')
    return ap


def groups_option(flag, sample_cfg):
    """(active, path of the pattern file or None = the default set) from the command line's value (None = not given, True = given
    bare) and the config's ``sample`` section (``groups``: true or a path); the flag wins"""
    value = flag if flag is not None else sample_cfg.get('groups')
    if value is None or value is False or value == '':
        return False, None
    return True, (None if value is True else str(value))


def add_groups_argument(ap):
    """``--groups [PATTERNS.yml]`` on a parser of ``build_parser``, whose own option set stays what it was"""
    ap.add_argument('--groups', nargs='?', const=True, default=None, metavar='PATTERNS.yml',
                    help='count the functional groups of the finished molecules on the device and write groups.npz and groups.json; '
                         'bare: the default pattern set configs/groups_default.yml (overrides sample.groups)')
    return ap


def kekulize_option(flag, sample_cfg):
    """whether to write the Kekulé files: the command line's flag (None = not given) wins over the config's ``sample.kekulize``"""
    return bool(flag if flag is not None else sample_cfg.get('kekulize'))


def add_kekulize_argument(ap):
    """``--kekulize`` on a parser of ``build_parser``, whose own option set stays what it was"""
    ap.add_argument('--kekulize', action='store_true', default=None,
                    help='assign a Kekulé structure to the aromatic bonds of the finished molecules on the device and write kekule.npz, '
                         'kekule.json and samples_kekule.sdf (overrides sample.kekulize)')
    return ap


def hydrogens_option(flag, clash_tol, sample_cfg):
    """whether to write the all-atom files, and the clash threshold of ``moldiff_amd/hydrogens.py`` in Angstrom: the command line
    (None = not given) wins over the config's ``sample.hydrogens`` and ``sample.clash_tol``; 1.5 where neither says -- a convention,
    untuned"""
    from . import hydrogens
    tol = float(clash_tol if clash_tol is not None else sample_cfg.get('clash_tol') if sample_cfg.get('clash_tol') is not None
                else hydrogens.DEFAULT_CLASH_TOL)
    return bool(flag if flag is not None else sample_cfg.get('hydrogens')), hydrogens._check(hydrogens.DEFAULT_DEG_TOL, tol)[1]


def add_hydrogens_argument(ap):
    """``--hydrogens`` on a parser of ``build_parser``, whose own option set stays what it was"""
    ap.add_argument('--hydrogens', action='store_true', default=None,
                    help='place the hydrogens of the Kekulé assignment on the finished molecules on the device and write hydrogens.npz, '
                         'hydrogens.json and samples_allatom.sdf; implies --kekulize (overrides sample.hydrogens)')
    ap.add_argument('--clash_tol', type=float, default=None,
                    help='a contact of a placed hydrogen below this many Angstrom is a clash (overrides sample.clash_tol; 1.5: a '
                         'convention, untuned)')
    return ap


def relax_option(flag, iters, gtol, sample_cfg):
    """whether to write the relaxation files, and the iteration limit and rms-gradient threshold of ``moldiff_amd/relax.py``: the command
    line (None = not given) wins over the config's ``sample.relax``, ``sample.relax_iters`` and ``sample.relax_gtol``; 200 and 1e-2
    kcal/mol/Angstrom where neither says"""
    from . import relax
    pick = lambda v, key, default: v if v is not None else sample_cfg.get(key) if sample_cfg.get(key) is not None else default
    iters, gtol = relax._check(pick(iters, 'relax_iters', relax.DEFAULT_MAX_ITERS), pick(gtol, 'relax_gtol', relax.DEFAULT_GTOL))[:2]
    return bool(flag if flag is not None else sample_cfg.get('relax')), iters, gtol


def add_relax_argument(ap):
    """``--relax`` on a parser of ``build_parser``, whose own option set stays what it was"""
    ap.add_argument('--relax', action='store_true', default=None,
                    help='relax the all-atom finished molecules in a UFF-form force field on the device and write relax.npz, relax.json '
                         'and samples_relaxed.sdf; implies --hydrogens (overrides sample.relax)')
    ap.add_argument('--relax_iters', type=int, default=None, help='L-BFGS iterations at most (overrides sample.relax_iters; 200)')
    ap.add_argument('--relax_gtol', type=float, default=None,
                    help='rms gradient in kcal/mol/Angstrom at which a molecule has converged (overrides sample.relax_gtol; 1e-2: a convention)')
    return ap


def global3d_option(n_confs, seed, sample_cfg):
    """how many conformers ``--global3d`` generates per finished molecule (0: off) and their seed: the command line (None = not given)
    wins over the config's ``sample.global3d`` and ``sample.global3d_seed``; the seed defaults to 0"""
    n = n_confs if n_confs is not None else sample_cfg.get('global3d')
    seed = seed if seed is not None else sample_cfg.get('global3d_seed')
    n, seed = int(n or 0), int(seed or 0)
    if not 0 <= n <= 65535 or seed < 0:
        raise ValueError(f'global3d must lie in 0 .. 65535 and its seed must not be negative, got {n} and {seed}')
    return n, seed


def add_global3d_argument(ap):
    """``--global3d`` on a parser of ``build_parser``, whose own option set stays what it was"""
    ap.add_argument('--global3d', type=int, default=None, metavar='N',
                    help='generate N conformers of every finished molecule on the device (distance geometry, then the relaxation), take the best '
                         'RMSD of each against the molecule and write global3d.npz, global3d.json and conformers.sdf; implies --hydrogens '
                         '(overrides sample.global3d)')
    ap.add_argument('--global3d_seed', type=int, default=None, help='seed of the starting coordinates (overrides sample.global3d_seed; 0)')
    return ap


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=str, required=True)
    ap.add_argument('--outdir', type=str, default='./outputs')
    ap.add_argument('--device', type=str, default='cuda:0')
    ap.add_argument('--batch_size', type=int, default=0)
    ap.add_argument('--recipe-weights', action='store_true')
    ap.add_argument('--num_mols', type=int, default=0, help='override sample.num_mols')
    ap.add_argument('--scaffold', type=str, default='', help='V2000 mol block held fixed as the first atoms of every molecule '
                                                             '(overrides sample.scaffold)')
    ap.add_argument('--num_steps', type=int, default=0, help='strided sampling: run the reverse chain on this many uniformly spaced '
                                                             'levels instead of all of them (overrides sample.num_steps)')
    ap.add_argument('--resample', type=int, default=0, help='resampling: walk every block of --jump_length levels this many times, with a '
                                                            'forward jump in between (overrides sample.resample; needs --jump_length)')
    ap.add_argument('--jump_length', type=int, default=0, help='resampling: moves per block (overrides sample.jump_length)')
    ap.add_argument('--accept', type=str, default=None, help="'connected' (one fragment), 'valence' (that and no over-valent atom) or "
                                                             "'kekule' (that and a Kekulé structure for every aromatic system); "
                                                             'judged by the device-side check (overrides sample.accept)')
    ap.add_argument('--largest_fragment', type=float, default=None,
                    help='FRAC in (0, 1]: a disconnected molecule whose largest fragment holds at least FRAC of its atoms is replaced '
                         'by that fragment before it is judged (overrides sample.largest_fragment; no default)')
    ap.add_argument('--local3d', type=str, default=None, help='pattern file (YAML: lengths / angles / dihedrals): accumulate the bond length / '
                                                              'angle / dihedral histograms of the finished molecules on the device and '
                                                              'write local3d.npz (overrides sample.local3d)')
    return ap


def canonical_option(flag, sample_cfg):
    """whether to write the canonical files: the command line's flag (None = not given) wins over the config's ``sample.canonical``"""
    return bool(flag if flag is not None else sample_cfg.get('canonical'))


def add_canonical_argument(ap):
    """``--canonical`` on a parser of ``build_parser``, whose own option set stays what it was"""
    ap.add_argument('--canonical', action='store_true', default=None,
                    help='label the finished molecules canonically on the device and write canon.npz and canon.json, with --kekulize '
                         'also samples.smi (overrides sample.canonical)')
    ap.add_argument('--canonical_max_nodes', type=int, default=None,
                    help='the node budget of the canonical search, 1 .. 2^20 (overrides sample.canonical_max_nodes; default 65536)')
    return ap


def stereo_option(flag, flat_tol, bond_tol, sample_cfg):
    """whether to write the stereo files, and the two thresholds of ``moldiff_amd/stereo.py``: the command line (None = not given) wins
    over the config's ``sample.stereo``, ``sample.stereo_flat_tol`` and ``sample.stereo_bond_tol``; 0.1 where neither says"""
    from . import stereo
    pick = lambda v, key, default: float(v if v is not None else sample_cfg.get(key) if sample_cfg.get(key) is not None else default)
    flat, bond = pick(flat_tol, 'stereo_flat_tol', stereo.DEFAULT_FLAT_TOL), pick(bond_tol, 'stereo_bond_tol', stereo.DEFAULT_BOND_TOL)
    stereo._check(flat, bond, 1)
    return bool(flag if flag is not None else sample_cfg.get('stereo')), flat, bond


def add_stereo_argument(ap):
    """``--stereo`` on a parser of ``build_parser``, whose own option set stays what it was"""
    ap.add_argument('--stereo', action='store_true', default=None,
                    help='perceive the stereo of the finished molecules on the device and write stereo.npz and stereo.json; implies '
                         '--canonical, and with --kekulize samples.smi is isomeric (overrides sample.stereo)')
    ap.add_argument('--stereo_flat_tol', type=float, default=None, help='the flatness threshold of a centre (overrides sample.stereo_flat_tol; 0.1)')
    ap.add_argument('--stereo_bond_tol', type=float, default=None, help='the cis / trans threshold (overrides sample.stereo_bond_tol; 0.1)')
    return ap


def conformers_option(flag, tol, sample_cfg):
    """whether to write the conformer files, and the RMSD in Angstrom up to which two conformers count as one
    (``moldiff_amd/rmsd.py``): the command line (None = not given) wins over the config's ``sample.conformers`` and
    ``sample.conformer_tol``; 0.5 where neither says -- a convention, not tuned"""
    from . import rmsd
    tol = float(tol if tol is not None else sample_cfg.get('conformer_tol') if sample_cfg.get('conformer_tol') is not None else rmsd.DEFAULT_TOL)
    return bool(flag if flag is not None else sample_cfg.get('conformers')), rmsd._check_tol(tol)


def add_conformers_argument(ap):
    """``--conformers`` on a parser of ``build_parser``, whose own option set stays what it was"""
    ap.add_argument('--conformers', action='store_true', default=None,
                    help='measure the best RMSD between the finished molecules of equal constitution on the device and write '
                         'conformers.npz and conformers.json; implies --canonical (overrides sample.conformers)')
    ap.add_argument('--conformer_tol', type=float, default=None,
                    help='two conformers are the same up to this RMSD in Angstrom (overrides sample.conformer_tol; 0.5: a convention, not tuned)')
    return ap


def frameworks_option(flag, generic, exo, sample_cfg):
    """whether to write the framework files, and the mode of ``moldiff_amd/framework.py``: the command line's flags (None = not given)
    win over the config's ``sample.frameworks``, ``sample.frameworks_generic`` and ``sample.frameworks_exo``"""
    pick = lambda f, key: bool(f if f is not None else sample_cfg.get(key))
    return pick(flag, 'frameworks'), (1 if pick(exo, 'frameworks_exo') else 0) | (2 if pick(generic, 'frameworks_generic') else 0)


def add_frameworks_argument(ap):
    """``--frameworks`` on a parser of ``build_parser``, whose own option set stays what it was"""
    ap.add_argument('--frameworks', action='store_true', default=None,
                    help='cut the finished molecules into framework, ring systems, linkers and side chains on the device and write '
                         'frameworks.npz and frameworks.json (overrides sample.frameworks)')
    ap.add_argument('--frameworks_generic', action='store_true', default=None,
                    help='frameworks and ring systems with every atom as class 0 and every bond single (overrides sample.frameworks_generic)')
    ap.add_argument('--frameworks_exo', action='store_true', default=None,
                    help='double-bonded atoms on the core join the framework (overrides sample.frameworks_exo)')
    return ap


def main(argv=None):
    args = add_global3d_argument(add_relax_argument(add_hydrogens_argument(add_conformers_argument(add_frameworks_argument(add_stereo_argument(add_canonical_argument(add_kekulize_argument(add_groups_argument(add_rings_argument(add_similarity_argument(build_parser()))))))))))).parse_args(argv)
    if args.accept is not None:
        accept_rule(args.accept)
    if args.largest_fragment is not None:
        fragment_fraction(args.largest_fragment)

    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    dist = None
    if world > 1:
        import torch.distributed as dist
        # one process per GPU over RCCL; MDX_DIST_BACKEND=gloo (ranks may then share a GPU) exists only so that the
        # multi-rank control flow can be exercised on a single-GPU test box
        backend = os.environ.get('MDX_DIST_BACKEND', 'nccl')
        lr = int(os.environ.get('LOCAL_RANK', '0'))
        args.device = f"cuda:{lr if backend == 'nccl' else lr % torch.cuda.device_count()}"
    device = torch.device(args.device)
    # the library allocates and launches on the CURRENT HIP device: make it the one the tensors live on (the reference's
    # default is --device cuda:7) before any handle is created
    torch.cuda.set_device(device)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=device)
        else:
            dist.init_process_group(backend)
    comm_dev = device if (world > 1 and backend == 'nccl') else torch.device('cpu')

    config = load_config(args.config)
    config_name = os.path.basename(args.config).rsplit('.', 1)[0]
    seed = int(config.sample.seed + np.sum([ord(s) for s in args.outdir]))
    seed_all(seed)
    log_dir = os.path.join(args.outdir, config_name + '_' + time.strftime('%Y%m%d_%H%M%S'))
    if world > 1:  # every rank writes trajectories of its own molecules: agree on rank 0's directory name
        name = [log_dir]
        dist.broadcast_object_list(name, src=0)   # once per run, not per batch
        log_dir = name[0]
    if rank == 0:
        os.makedirs(log_dir, exist_ok=True)
        shutil.copyfile(args.config, os.path.join(log_dir, os.path.basename(args.config)))
    os.makedirs(log_dir + '_SDF', exist_ok=True)
    featurizer = FeaturizeMol([6, 7, 8, 9, 15, 16, 17], [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
    model, bond_predictor, guidance = build_models(config, device, args.recipe_weights)
    num_mols = args.num_mols or config.sample.num_mols
    batch_size = args.batch_size if args.batch_size > 0 else config.sample.batch_size
    save_traj_prob = float(getattr(config.sample, 'save_traj_prob', 0.0) or 0.0)
    scaffold_path = args.scaffold or config.sample.get('scaffold') or ''
    num_steps = args.num_steps or config.sample.get('num_steps') or None   # trajectory files then hold num_steps + 1 frames
    # resampling: trajectory files then hold one frame per move + 1 (schedule.resampling_path), up-moves included
    resample = args.resample or config.sample.get('resample') or None
    jump_length = args.jump_length or config.sample.get('jump_length') or None
    extra = {} if num_steps is None else {'num_steps': int(num_steps)}
    if resample is not None or jump_length is not None:
        extra.update(resample=None if resample is None else int(resample), jump_length=None if jump_length is None else int(jump_length))
    rule, frac, checked = quality_options(args.accept, args.largest_fragment, config.sample)
    local3d_path = local3d_option(args.local3d, config.sample)
    l3d_spec, l3d_stats = None, None
    if local3d_path:   # read on every rank, so that a bad file stops all of them
        from . import local3d
        l3d_spec = local3d.Local3DSpec.from_yaml(local3d_path)
    sim_active, sim_ref_path = similarity_option(args.similarity, config.sample)
    sim_spec, sim_set, sim_ref = None, None, None
    if sim_active:   # read on every rank, so that a bad file stops all of them
        from . import similarity
        sim_spec = similarity.FingerprintSpec(atomic_numbers=featurizer.atomic_numbers.tolist(), num_bond_types=featurizer.num_bond_types)
        if sim_ref_path:
            sim_ref = similarity.FingerprintSet.load(sim_ref_path)
            if sim_ref.spec != sim_spec:
                raise ValueError(f'{sim_ref_path} was made with another spec ({sim_ref.spec.to_dict()}) than this run\'s ({sim_spec.to_dict()})')
    Z, nbt = featurizer.atomic_numbers.tolist(), featurizer.num_bond_types
    features = []   # in the order their files are written
    if rings_option(args.rings, config.sample):
        from . import rings
        features.append(Feature(lambda gen: rings.rings_mols(gen, device, nbt, Z), rings, 'rings', empty=lambda: rings.empty(nbt, Z)))
    groups_active, groups_path = groups_option(args.groups, config.sample)
    if groups_active:   # read on every rank, so that a bad file stops all of them
        from . import groups
        groups_set = groups.PatternSet.from_yaml(groups_path, Z, nbt) if groups_path else groups.PatternSet.default(Z, nbt)
        features.append(Feature(lambda gen: groups.groups_mols(gen, device, groups_set), groups, 'groups', empty=lambda: groups.empty(groups_set)))
    hydrogens_on, clash_tol = hydrogens_option(args.hydrogens, args.clash_tol, config.sample)
    relax_on, relax_iters, relax_gtol = relax_option(args.relax, args.relax_iters, args.relax_gtol, config.sample)
    g3d_confs, g3d_seed = global3d_option(args.global3d, args.global3d_seed, config.sample)
    hydrogens_on = hydrogens_on or relax_on or g3d_confs > 0   # --relax and --global3d imply --hydrogens
    kek_write = kekulize_option(args.kekulize, config.sample) or hydrogens_on   # --hydrogens implies --kekulize
    kek_active = kek_write or rule == 'kekule'
    if kek_active:
        from . import kekule
        kek_tables = kekule.KekuleTables(Z, nbt)
    if kek_write:
        kek_held = {}   # the joined Kekulé results, for the all-atom file of --hydrogens

        def write_kekule_sdf(res):
            kek_held['kekule'] = res
            kekule.write_sdf(os.path.join(log_dir, 'samples_kekule.sdf'), pool['finished'], res)
        features.append(Feature(lambda gen: kekule.kekulize_mols(gen, device, kek_tables), kekule, 'kekule', after=write_kekule_sdf))
    if hydrogens_on:   # behind kekule: the joined Kekulé results are there when the all-atom file is written
        from . import hydrogens
        h_tables = hydrogens.HydrogenTables(Z, nbt)

        def write_allatom_sdf(res):
            kek_held['hydrogens'] = res
            hydrogens.write_sdf(os.path.join(log_dir, 'samples_allatom.sdf'), pool['finished'], kek_held['kekule'], res)
        features.append(Feature(lambda gen: hydrogens.addh_mols(gen, device, tables=h_tables, clash_tol=clash_tol), hydrogens, 'hydrogens',
                                summary=lambda res: hydrogens.summary(res, clash_tol), after=write_allatom_sdf))
    if relax_on:   # behind hydrogens: the joined Kekulé and hydrogen results are there when the relaxed file is written
        from . import relax
        ff_tables = relax.ForceFieldTables(Z, nbt)
        features.append(Feature(lambda gen: relax.relax_mols(gen, device, ff_tables, relax_iters, relax_gtol), relax, 'relax',
                                after=lambda res: relax.write_sdf(os.path.join(log_dir, 'samples_relaxed.sdf'), pool['finished'],
                                                                  kek_held['kekule'], kek_held['hydrogens'], res)))
    if g3d_confs:   # behind hydrogens: the joined Kekulé and hydrogen results are there when the conformers are written
        from . import embed
        g3d_tables = embed.relax.ForceFieldTables(Z, nbt)
        features.append(Feature(lambda gen: embed.global3d_mols(gen, device, g3d_confs, g3d_seed, g3d_tables, mol_ids=[int(m['mol_id']) for m in gen]),
                                embed, 'global3d', empty=lambda: embed.empty(g3d_confs),
                                after=lambda res: embed.write_sdf(os.path.join(log_dir, 'conformers.sdf'), pool['finished'], kek_held['kekule'],
                                                                  kek_held['hydrogens'], res)))
    stereo_on, flat_tol, bond_tol = stereo_option(args.stereo, args.stereo_flat_tol, args.stereo_bond_tol, config.sample)
    conformers_on, conformer_tol = conformers_option(args.conformers, args.conformer_tol, config.sample)
    if canonical_option(args.canonical, config.sample) or stereo_on or conformers_on:
        from . import canon, stereo
        held = {}   # the stereo part of the batch at hand, and the joined canon results for the stereo summary
        canon_nodes = args.canonical_max_nodes or config.sample.get('canonical_max_nodes') or canon.DEFAULT_MAX_NODES
        if not 1 <= canon_nodes <= canon.MAX_NODES_LIMIT:
            raise ValueError(f'canonical_max_nodes must lie in 1 .. 2^20, got {canon_nodes}')

        def run_canon(gen):
            if stereo_on:
                part, held['stereo'] = (to_host(r) for r in stereo.stereo_mols(gen, device, None, flat_tol, bond_tol, max_nodes=canon_nodes,
                                                                                 atomic_numbers=Z, with_canon=True))
            else:
                part = to_host(canon.canon_mols(gen, device, max_nodes=canon_nodes, atomic_numbers=Z))
            if kek_write:   # the strings need the canonical part and the Kekulé tables of the same batch
                for info, text in zip(gen, canon.smiles_mols(gen, part, device, kek_tables, held.get('stereo'))):
                    info['smiles'] = text
            return part

        def write_smi(res):
            held['canon'] = res
            if kek_write:
                with open(os.path.join(log_dir, 'samples.smi'), 'w') as f:
                    f.writelines('%s\t%d\n' % (m['smiles'], m['mol_id']) for m in pool['finished'] if m.get('smiles'))
        features.append(Feature(run_canon, canon, 'canon', after=write_smi))
        if stereo_on:   # behind canon: its batch part is there, and so are the joined canon results when the summary is written
            features.append(Feature(lambda gen: held.pop('stereo'), stereo, 'stereo',
                                    summary=lambda res: dict(stereo.summary(res, held['canon']), flat_tol=flat_tol, bond_tol=bond_tol)))
    fw_write, fw_mode = frameworks_option(args.frameworks, args.frameworks_generic, args.frameworks_exo, config.sample)
    if fw_write:
        from . import framework
        fw_nodes = args.canonical_max_nodes or config.sample.get('canonical_max_nodes') or framework.canon.DEFAULT_MAX_NODES
        features.append(Feature(lambda gen: framework.stats_mols(gen, device, fw_mode, max_nodes=fw_nodes, atomic_numbers=Z, num_bond_types=nbt),
                                framework, 'frameworks', empty=lambda: framework.empty(with_keys=True),
                                summary=lambda res: dict(framework.summary(res, device=device, atomic_numbers=Z), mode=fw_mode)))
    parts = [[] for _ in features]
    scaffold_info = None
    if scaffold_path:
        with open(scaffold_path) as f:
            scaffold_info = read_mol_block(f.read())
    pool = {'finished': [], 'failed': []}
    n_finished, n_failed = 0, 0
    next_id, i_batch = 0, 0
    while n_finished < num_mols:
        if n_failed > 3 * num_mols:
            if rank == 0:
                print('Too many failed molecules. Stop sampling.')
            break
        n_graphs = min(batch_size, (num_mols - n_finished) * 2)
        # every rank draws the same sizes (same numpy stream) and takes a contiguous slice of the cost-balanced order
        sizes = np.random.normal(GEOM_DRUGS_MEAN_ATOMS, GEOM_DRUGS_STD_ATOMS, size=n_graphs).astype('int64')
        sizes = np.maximum(sizes, 2)  # the reference's harness cannot handle molecules without half-edges
        if scaffold_info is not None:
            sizes = np.maximum(sizes, len(scaffold_info['element']))
        order = balanced_order(sizes, world) if world > 1 else np.arange(n_graphs)
        lo, hi = shard_bounds(n_graphs, world, rank)
        mine = order[lo:hi]
        ph = placeholder_from_sizes(sizes[mine], device)
        ids = next_id + mine.astype(np.int64)
        # each rank builds the scaffold of its own slice; its noise is keyed by global molecule id like the chain's
        scaffold = scaffold_for_sizes(scaffold_info, sizes[mine], featurizer, device) if scaffold_info is not None else None
        out = model.sample(hi - lo, ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge'], bond_predictor, guidance,
                           seed=seed + i_batch, mol_ids=ids, return_traj=save_traj_prob > 0, scaffold=scaffold,
                           **extra)
        # trajectories stay rank-local (scripts/sample_drug3d.py:155 looks at ~2 % of them): the owner decodes and writes
        # them, named by global molecule id; whether a molecule is drawn depends only on (seed, id), not on the sharding
        if save_traj_prob > 0:
            if checked:   # the same rule as rank 0 below: a function of the molecule alone
                local, rep = featurizer.check_batch(out['pred'], ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge'], hi - lo,
                                                    largest_fragment=frac)
                done = [judge(info, rep, j, rule)[0] for j, info in enumerate(local)]
                if rule == 'kekule':
                    ok = kekule.kekulizable(kekule.kekulize_mols(local, device, kek_tables))
                    done = [d and bool(k) for d, k in zip(done, ok)]
            else:
                local = featurizer.decode_batch(out['pred'], ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge'], hi - lo)
                done = [is_connected(len(info['element']), info['bond_index']) for info in local]
            sel = [j for j, info in enumerate(local)
                   if done[j]
                   and np.random.default_rng([seed, int(ids[j])]).random() < save_traj_prob]
            if sel:
                for j, frames in traj_blocks(featurizer, out['traj'], sel, sizes[mine], device).items():
                    path = os.path.join(log_dir + '_SDF', 'traj_mol%d.sdf' % int(ids[j]))
                    with open(path, 'w') as f:
                        for info in frames:
                            f.write(mol_block(info) + '$$$$\n')
        # the only data-path collective: this batch's last-step predictions to rank 0 (one count all_gather + one padded
        # gather-to-rank-0 of a flat buffer, RCCL over xGMI; about 2 MB per rank at 256 molecules)
        pred = out['pred']
        if dist is not None:
            pred = gather_pred([p.to(comm_dev) for p in pred], dst=0)
        counts = torch.zeros(2, dtype=torch.int64, device=comm_dev)
        if rank == 0:
            full = placeholder_from_sizes(sizes[order], device)
            inv = np.argsort(order)                       # back to the batch's original molecule order
            if checked:
                mols, rep = featurizer.check_batch([p.to(device) for p in pred], full['batch_node'], full['halfedge_index'],
                                                   full['batch_halfedge'], n_graphs, largest_fragment=frac)
                done = [judge(mols[inv[k]], rep, inv[k], rule, annotate=True)[0] for k in range(n_graphs)]
            else:
                mols = featurizer.decode_batch([p.to(device) for p in pred], full['batch_node'], full['halfedge_index'],
                                               full['batch_halfedge'], n_graphs)
            mols = [mols[inv[k]] for k in range(n_graphs)]
            if kek_active:   # of every molecule as it stands (with --largest_fragment a salvaged molecule is its fragment)
                ok = kekule.kekulizable(kekule.kekulize_mols(mols, device, kek_tables))
                for k, info in enumerate(mols):
                    info['kekulizable'] = bool(ok[k])
                if rule == 'kekule':
                    done = [d and bool(k) for d, k in zip(done, ok)]
            gen = []
            for k, info in enumerate(mols):
                info['mol_id'] = next_id + k
                if done[k] if checked else is_connected(len(info['element']), info['bond_index']):
                    gen.append(info)
                else:
                    pool['failed'].append(info)
            for i, info in enumerate(gen):
                with open(os.path.join(log_dir + '_SDF', '%d.sdf' % (i + len(pool['finished']))), 'w') as f:
                    f.write(mol_block(info) + '$$$$\n')
                # whether a finished molecule's trajectory was written is a function of (seed, global id) and of its connectivity
                # (tested above) -- not of the rank that sampled it: rank 0 re-derives the file name its owner used, so every
                # selected molecule carries its trajectory like in the reference (scripts/sample_drug3d.py:155-190)
                if save_traj_prob > 0 and np.random.default_rng([seed, int(info['mol_id'])]).random() < save_traj_prob:
                    info['traj_file'] = 'traj_mol%d.sdf' % info['mol_id']
            pool['finished'].extend(gen)
            if l3d_spec is not None:
                l3d_stats = local3d.local3d_mols(gen, l3d_spec, device, out=l3d_stats)
            if sim_spec is not None:
                fps = similarity.fingerprint_mols(gen, sim_spec, device)
                sim_set = fps if sim_set is None else sim_set.append(fps)
            if gen:
                for f, done_parts in zip(features, parts):
                    done_parts.append(to_host(f.run(gen)))
            print('[Pool] Finished %d | Failed %d' % (len(pool['finished']), len(pool['failed'])))
            counts[0], counts[1] = len(pool['finished']), len(pool['failed'])
        if dist is not None:  # one small all-reduce keeps the loop condition identical on every rank
            dist.all_reduce(counts)
        n_finished, n_failed = int(counts[0]), int(counts[1])
        next_id += n_graphs
        i_batch += 1
    if rank == 0:
        torch.save(pool, os.path.join(log_dir, 'samples_all.pt'))
        if l3d_spec is not None:
            (l3d_stats or local3d.device_stats(l3d_spec, device)).save(os.path.join(log_dir, 'local3d.npz'))
        if sim_spec is not None:
            sim_set = sim_set if sim_set is not None else similarity.FingerprintSet.empty(sim_spec).to(device)
            sim_set.save(os.path.join(log_dir, 'fingerprints.npz'))
            with open(os.path.join(log_dir, 'similarity.json'), 'w') as f:
                json.dump(similarity.summary(sim_set, sim_ref.to(device) if sim_ref is not None else None), f, indent=1)
        for f, done_parts in zip(features, parts):
            res = f.module.concat(done_parts) if done_parts else (f.empty or f.module.empty)()
            save_npz(res, os.path.join(log_dir, f.stem + '.npz'))
            with open(os.path.join(log_dir, f.stem + '.json'), 'w') as fh:
                json.dump((f.summary or f.module.summary)(res), fh, indent=1)
            if f.after is not None:
                f.after(res)
        if conformers_on:   # over the whole pool at once: the groups of equal constitution run across the batches
            from . import rmsd
            res = rmsd.conformer_results(pool['finished'], None, conformer_tol, device=device, max_nodes=canon_nodes, atomic_numbers=Z)
            save_npz(res, os.path.join(log_dir, 'conformers.npz'))
            with open(os.path.join(log_dir, 'conformers.json'), 'w') as fh:
                json.dump(rmsd.summary(res), fh, indent=1)
        if checked:
            with open(os.path.join(log_dir, 'quality.json'), 'w') as f:
                json.dump(dict(quality_summary(pool['finished'] + pool['failed'], len(pool['finished']), len(pool['failed']),
                                               kekule=kek_active),
                               accept=rule, largest_fragment=frac), f, indent=1)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return log_dir


if __name__ == '__main__':
    main()
