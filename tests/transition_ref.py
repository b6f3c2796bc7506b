"""Float64 restatement of the row formulas of csrc/mdx_transition.hip, on the host, and the fixed inputs the GPU tests of
tests/test_gpu_transition_fp64.py run them on (tests/test_transition_ref_host.py checks the caps for exactly these inputs).

Every function takes the project's STORED fp32 tables (widened here) and evaluates the reference's formula (models/transition.py,
models/diffusion.py, models/model.py:170-189 and :322-324) in float64 with plain torch-CPU operators.  `posterior_fp64`, `classes_fp64`,
`MARGIN` and `SKIP_CAP` are those of tests/test_schedule_host.py.  The functions that also serve as the fp32 yardstick (the loss tail,
the uncertainty gradient) take the dtype as an argument: the SAME torch expression evaluated in float32 on the CPU is the "fp32
reference" whose distance from float64 the GPU tests scale their tolerances by.  No GPU needed."""
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

import moldiff_amd as M
from moldiff_amd.harness import default_config
from oracle import moldiff_oracle as O
from tests import util as U
from tests.test_schedule_host import MARGIN, SKIP_CAP, classes_fp64, posterior_fp64   # noqa: F401  (re-exported)

T = 1000
KS = (2, 3, 4, 5, 6, 7, 8)
ROWS = (1, 255, 256, 257, 1000)          # one row; one short of / exactly / one past a block of 256 (two of 128); several blocks
SCALES = (0.3, 3.0, 40.0)
WIDTHS = (1, 3, 5, 8, 64)                # row widths C of the Gaussian posterior
NEAR = 1e-3                              # a loss row is flagged when a clamp input lies within this of -32
FLAG_CAP = 0.005                         # ... and at most this share of the loss rows may be flagged
B, EMPTY = 7, 3                          # molecules per launch; molecule EMPTY owns no row
U24 = 2.0 ** -24


def ulp32(x):
    """spacing of fp32 at magnitude |x| (a float64 tensor or number): 2^(floor(log2 |x|) - 23), the smallest normal's below that"""
    x = torch.as_tensor(x, dtype=torch.float64).abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(x)) - 23.0)


# ---- transitions ----------------------------------------------------------------------------------------------------------------------
# K = 8 / 6: MolDiff's node / edge transition.  Other class counts through the project's own constructor, the way
# test_other_class_counts_take_the_standalone_jump_launches builds its model: 'tomask' (node) and 'absorb' (edge) priors both occur.
_OTHER = {7: ((7, 5), 'node'), 5: ((7, 5), 'edge'), 3: ((3, 4), 'node'), 4: ((3, 4), 'edge'), 2: ((2, 2), 'node')}
_other_models = {}


def other_model(kn, ke):
    """MolDiff_simple with (kn, ke) classes and recipe weights, on the CPU"""
    if (kn, ke) not in _other_models:
        mk = M.MolDiff(copy.deepcopy(default_config('MolDiff_simple')), kn, ke).eval()
        mk.load_state_dict(M.recipe_state_dict(mk, 99), strict=True)
        _other_models[(kn, ke)] = mk
    return _other_models[(kn, ke)]


TABLES = ('model', 'sparse')


@functools.lru_cache(maxsize=None)
def transition(K, tables='model'):
    """the GeneralCategoricalTransition with K classes (CPU).  'model': the shipped one.  Its smallest table entry is 1e-7, so with a
    normalised v0_hat and a one-hot v_t neither log(f + 1e-30) of the posterior can come near -32: the clamp never acts.  'sparse': the
    same constructor and beta schedule with a prior that is 1e-13 on all classes but the last.  Then Q[j,k] = (1 - abar) 1e-13 falls
    under e^-32 = 1.27e-14 at the lower levels and stays above it at the upper ones: both sides of the clamp, and of the backward's
    gate, occur."""
    if tables == 'sparse':
        from moldiff_amd.transition import GeneralCategoricalTransition
        p0 = np.full(K, 1e-13)
        p0[-1] = 1.0
        return GeneralCategoricalTransition(transition(K).betas, K, init_prob=p0)
    if K == 8:
        return U.moldiff('MolDiff').node_transition
    if K == 6:
        return U.moldiff('MolDiff').edge_transition
    (kn, ke), part = _OTHER[K]
    mk = other_model(kn, ke)
    return mk.node_transition if part == 'node' else mk.edge_transition


# ---- the float64 formulas -------------------------------------------------------------------------------------------------------------

def posterior64(Q0_rows, Q1T_rows, in0, log_vt, last, is_logits):
    """log q(v_s | v_t, v0_hat) per row.  Q0_rows (n,K,K): the row's cumulative matrix Qbar_s; Q1T_rows (n,K,K): the row's transposed
    forward matrix from s to t; in0: logits (is_logits) or log-probabilities log v0_hat; last (n,) bool: the row's t == 0, where the
    result is log v0_hat itself.  log(f + 1e-30).clamp_min(-32) on both factors, normalised (models/transition.py:285-315).
    The logits form IS tests/test_schedule_host.py's posterior_fp64 (every row its own table row); the log-probability form states the
    same expression on in0 as given: the kernel does not re-normalise it."""
    n = in0.shape[0]
    rows = torch.arange(n)
    if is_logits:
        return posterior_fp64(Q0_rows, Q1T_rows, in0, log_vt, torch.where(last, 0, 1), rows, rows)
    l0 = in0.double()
    f1 = (log_vt.double().exp().unsqueeze(-1) * Q1T_rows.double()).sum(dim=1)
    f2 = (l0.exp().unsqueeze(-1) * Q0_rows.double()).sum(dim=1)
    out = torch.log(f1 + 1e-30).clamp_min(-32.0) + torch.log(f2 + 1e-30).clamp_min(-32.0)
    out = out - torch.logsumexp(out, dim=-1, keepdim=True)
    return torch.where(last.unsqueeze(-1), l0, out)


def onestep_rows(tr, t, batch):
    """(Q0_rows, Q1T_rows, last) of the chain's ordinary move t -> t - 1 for rows of molecules `batch` at levels t"""
    tb = t[batch]
    return tr.q_mats.detach()[(tb - 1).clamp(min=0)], tr.transpopse_q_onestep_mats.detach()[tb], tb == 0


def gauss64(c0, ct, sd, x0, xt, eps, last):
    """c0 x0 + ct xt (+ sd eps unless last) with per-row coefficients (n,) and rows (n,C) -> (value, rounding bound of an fp32 evaluation
    without contraction): the kernel rounds a = c0 x0, b = ct xt, a + b, c = sd eps and (a + b) + c once each, so
    |err| <= 2^-24 (|a| + |b| + |a + b| + |c| + |a + b + c|) <= 3 * 2^-24 (|a| + |b| + |c|) to first order, second order in (1 + 2^-20);
    rows at t == 0 have no noise term, in the value and in the bound."""
    a, b, c = (k.double().unsqueeze(-1) * x.double() for k, x in ((c0, x0), (ct, xt), (sd, eps)))
    c = torch.where(last.unsqueeze(-1), torch.zeros_like(c), c)
    return a + b + c, 3 * U24 * (a.abs() + b.abs() + c.abs()) * (1 + 2.0 ** -20)


def gumbel_classes64(logp, u):
    """argmax_k(logp - log(-log(u + 1e-30) + 1e-30)) in float64 -> (class, margin between the two best scores)"""
    return classes_fp64(logp.double(), u)


def uncertainty_grad(logits, dtype=torch.float64):
    """d/d logits of log sigmoid(-logsumexp(logits)) (models/model.py:322-324) = -sigmoid(lse) softmax(logits) -> (gradient, lse)"""
    x = logits.to(dtype)
    lse = torch.logsumexp(x, dim=-1, keepdim=True)
    return -torch.sigmoid(lse) * torch.softmax(x, dim=-1), lse.squeeze(-1)


def uncertainty_grad64(logits):
    return uncertainty_grad(logits)[0]


def add_noise64(Q_row, v, u):
    """q(v_t | v_0) draw (models/transition.py:266-283): Q_row (n,K,K) = q_mats[t] per row, v (n,) class ids (clamped into 0..K-1, as
    the kernel documents), u (n,K) uniforms -> (class, margin, log_v0) with log_v0 = log(clamp(onehot(v), 1e-30))"""
    K = Q_row.shape[-1]
    log_v0 = torch.log(F.one_hot(v.clamp(0, K - 1), K).double().clamp(min=1e-30))
    logits = torch.log((log_v0.exp().unsqueeze(-1) * Q_row.double()).sum(dim=1) + 1e-30).clamp_min(-32.0)
    cls, margin = classes_fp64(logits, u)
    return cls, margin, log_v0


def cat_loss_tail(q_mats, qT, logits, log_vt, log_v0, t, batch, dtype=torch.float64):
    """The categorical loss rows (models/model.py:170-189, models/transition.py:285-327) and d sum(rows) / d logits by torch autograd on
    the CPU in `dtype`: log_recon = log_softmax(logits); post_true / post_pred = q(v_{t-1} | v_t, log_v0 / log_recon); row =
    KL(post_true || post_pred) for t > 0, -sum exp(log_v0) post_pred at t == 0.
    -> (row_loss, dlogits, near, gated): near = some input of a clamp_min(-32) lies within NEAR of -32 (the clamp's gradient jumps
    there), gated = the row has a class whose f2 of the PREDICTED posterior lies under the clamp (its gradient path is cut)."""
    x = logits.detach().to(dtype).requires_grad_(True)
    lvt, lv0 = log_vt.to(dtype), log_v0.to(dtype)
    tb = t[batch]
    Q1, Q0 = qT.detach().to(dtype)[tb], q_mats.detach().to(dtype)[(tb - 1).clamp(min=0)]
    last = (tb == 0).unsqueeze(-1)
    lr = torch.log_softmax(x, dim=-1)
    a_in = torch.log((lvt.exp().unsqueeze(-1) * Q1).sum(dim=1) + 1e-30)

    def post(l0):
        b_in = torch.log((l0.exp().unsqueeze(-1) * Q0).sum(dim=1) + 1e-30)
        out = a_in.clamp_min(-32.0) + b_in.clamp_min(-32.0)
        return torch.where(last, l0, out - torch.logsumexp(out, dim=-1, keepdim=True)), b_in

    pt, bt_in = post(lv0)
    pp, bp_in = post(lr)
    kl = (pt.exp() * (pt - pp)).sum(dim=-1)
    nll = -(lv0.exp() * pp).sum(dim=-1)
    mask = (tb == 0).to(dtype)
    row = mask * nll + (1 - mask) * kl
    (g,) = torch.autograd.grad(row.sum(), x)
    with torch.no_grad():
        near = sum(((c + 32.0).abs() < NEAR).any(dim=-1) for c in (a_in, bt_in, bp_in)) > 0
        near = near & ~last.squeeze(-1)                     # at t == 0 the clamped factors are not part of the row
        gated = (bp_in < -32.0).any(dim=-1) & ~last.squeeze(-1)
    return row.detach(), g, near, gated


def cat_loss64(q_mats, qT, logits, log_vt, log_v0, t, batch):
    return cat_loss_tail(q_mats, qT, logits, log_vt, log_v0, t, batch)[:3]


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------------

def rows_case(n, seed):
    """(t (B,), batch (n,) sorted): B = 7 molecules at levels 0, 1, 2, T - 1 and random ones, molecule EMPTY without rows, every other
    molecule with at least one row once n >= 6 (so every such launch has t == 0 and t == 1 rows).  A single row lies at t == 1."""
    g = U.rng(seed)
    t = torch.tensor([0, 1, 2, 0, T - 1, 0, 0])
    t[[EMPTY, 5, 6]] = torch.from_numpy(g.integers(3, T - 1, 3))
    live = np.array([b for b in range(B) if b != EMPTY])
    if n < len(live):
        batch = live[1:1 + n]
    else:
        batch = np.sort(np.concatenate([live, g.choice(live, n - len(live))]))
    return t, torch.from_numpy(np.ascontiguousarray(batch, dtype=np.int64))


def log_onehot32(cls, K):
    """log(clamp(onehot, 1e-30)) as torch evaluates it in fp32: the chain's real log rows"""
    return torch.log(F.one_hot(cls, K).float().clamp(min=1e-30))


def posterior_case(K, n, scale, vt_form):
    """inputs of one cat_posterior launch: logits of the given scale, log v_t soft (log-softmax of 3 randn) or real (log one-hot),
    uniforms for the Gumbel draw on the result"""
    seed = 100000 * K + 100 * n + 10 * SCALES.index(scale) + (vt_form == 'real')
    g = U.rng(seed)
    t, batch = rows_case(n, seed + 5)
    logits = U.t32(scale * g.standard_normal((n, K)))
    if vt_form == 'soft':
        log_vt = F.log_softmax(U.t32(3.0 * g.standard_normal((n, K))), dim=-1)
    else:
        log_vt = log_onehot32(torch.from_numpy(g.integers(0, K, n)), K)
    return {'t': t, 'batch': batch, 'logits': logits, 'log_vt': log_vt, 'u': U.t32(g.random((n, K), dtype=np.float32))}


def gauss_case(C, n):
    g = U.rng(7000 + 10 * n + C)
    t, batch = rows_case(n, 7100 + n)
    x0, xt, eps = (U.t32(s * g.standard_normal((n, C))) for s in (2.0, 2.0, 1.0))
    return {'t': t, 'batch': batch, 'x0': x0, 'xt': xt, 'eps': eps}


SATURATED = (-45.0, -60.0, -100.0, -300.0)   # logit levels of the rows appended to every uncertainty input: lse below -40


def uncertainty_case(K, n, scale):
    """logits of the given scale, plus len(SATURATED) rows whose lse lies below -40 (sigmoid underflows towards 0; at -100 and below
    expf(-lse) overflows in fp32)"""
    g = U.rng(9000 + 100 * K + n + SCALES.index(scale))
    x = scale * g.standard_normal((n, K))
    sat = np.asarray(SATURATED)[:, None] + g.standard_normal((len(SATURATED), K))
    return U.t32(np.concatenate([x, sat]))


def noise_case(K, n):
    g = U.rng(11000 + 100 * K + n)
    t, batch = rows_case(n, 11500 + n)
    return {'t': t, 'batch': batch, 'v': torch.from_numpy(g.integers(0, K, n)), 'u': U.t32(g.random((n, K), dtype=np.float32))}


def loss_case(K, n, tables='model'):
    """clean classes v, their q(v_t | v_0) draw (the float64 reference's own class), logits with a per-row scale out of SCALES"""
    g = U.rng(13000 + 100 * K + n)
    t, batch = rows_case(n, 13500 + n)
    tr = transition(K, tables)
    v = torch.from_numpy(g.integers(0, K, n))
    cls, _, _ = add_noise64(tr.q_mats.detach()[t[batch]], v, U.t32(g.random((n, K), dtype=np.float32)))
    scale = torch.from_numpy(g.choice(SCALES, n)).float().unsqueeze(-1)
    return {'t': t, 'batch': batch, 'logits': U.t32(g.standard_normal((n, K))) * scale, 'log_vt': log_onehot32(cls, K),
            'log_v0': log_onehot32(v, K)}


# ---- the three index regimes of the fused step kernels ----------------------------------------------------------------------------------
FUSED_SIZES = {'Eh<N': [1, 1, 2, 1], 'N<Eh<3N': [3, 4, 0, 5], 'Eh>3N': [12, 9]}


# ---- references of the GPU tests: float64 value and the fp32 CPU evaluation's distance from it, computed once ---------------------------
def oracle32_rows(Q0_rows, Q1T_rows, last, log_v0, log_vt):
    """the fp32 CPU oracle's cat_posterior with every row its own table row (the same gather-then-einsum arithmetic): row i is handed
    "level" i + 1 of a table stack built from the rows, rows at t == 0 level 0 (the oracle returns log_v0 there)"""
    n = log_v0.shape[0]
    tab = {'q_mats': Q0_rows, 'transpopse_q_onestep_mats': torch.cat([Q1T_rows[:1], Q1T_rows])}
    lvl = torch.where(last, torch.zeros(n, dtype=torch.int64), torch.arange(1, n + 1))
    return O.cat_posterior(tab, log_v0, log_vt, lvl, torch.arange(n))


def posterior_reference(K, case, is_logits, tables='model', rows=None):
    """-> (in0 handed to the kernel, float64 posterior, last, max |fp32 CPU oracle - float64|) for one posterior_case; rows = (Q0_rows,
    Q1T_rows, last), by default those of the chain's ordinary move"""
    Q0, Q1, last = rows if rows is not None else onestep_rows(transition(K, tables), case['t'], case['batch'])
    log_v0 = F.log_softmax(case['logits'], dim=-1)              # fp32, CPU: what the oracle and the log-probability form are given
    in0 = case['logits'] if is_logits else log_v0
    ref = posterior64(Q0, Q1, in0, case['log_vt'], last, is_logits)
    o32 = oracle32_rows(Q0, Q1, last, log_v0, case['log_vt'])
    return in0, ref, last, float((o32.double() - ref).abs().max())


def jump_levels(t):
    """a level below every molecule's t: -1 under 0, 0 under 1 and 2, far below T - 1, and for the random levels a stride of 1, a
    jump to the middle and a jump onto 0"""
    s = torch.tensor([-1, 0, 0, 0, 420, 0, 0])
    s[EMPTY], s[5], s[6] = t[EMPTY] - 1, t[5] - 1, t[6] // 2
    return s


@functools.lru_cache(maxsize=None)
def gumbel_reference(K):
    """per row count: (fp32 rounding of the float64 posterior, uniforms, float64 class, margin)"""
    out = []
    for n in ROWS:
        case = posterior_case(K, n, 3.0, 'real')
        logp = posterior_reference(K, case, True)[1].float()
        out.append((logp, case['u']) + gumbel_classes64(logp, case['u']))
    return out


@functools.lru_cache(maxsize=None)
def gumbel_edge_rows(K):
    """rows whose uniforms hold the extremes of the noise kernel's u01 (0 and 1 - 2^-24), and rows with two bit-equal best scores (the
    tie must go to the lower index, like torch.argmax) -> (logp, u, float64 class / the tie's lower index, margin; is_tie)"""
    g = U.rng(15000 + K)
    n = 64
    logp = F.log_softmax(U.t32(g.standard_normal((n, K))), dim=-1)
    u = U.t32(g.random((n, K), dtype=np.float32))
    lo = g.integers(0, K, n)
    hi = (lo + 1 + g.integers(0, K - 1, n)) % K                         # another column than lo
    u[torch.arange(n), torch.from_numpy(lo)] = 0.0
    u[torch.arange(n), torch.from_numpy(hi)] = 1.0 - 2.0 ** -24
    cls, margin = gumbel_classes64(logp, u)
    # ties: columns a < b carry the same log-probability and the same uniform; every other column is far below
    tie_logp = torch.full((K * (K - 1) // 2, K), -20.0)
    tie_u = torch.full_like(tie_logp, 0.3)
    want = []
    for r, (a, b) in enumerate((a, b) for a in range(K) for b in range(a + 1, K)):
        tie_logp[r, [a, b]] = -0.75
        tie_u[r, [a, b]] = 0.625
        want.append(a)
    return logp, u, cls, margin, tie_logp, tie_u, torch.tensor(want)


@functools.lru_cache(maxsize=None)
def noise_reference(K):
    """per table set and row count: (tables, case, float64 class, margin, log_v0)"""
    out = []
    for tables in TABLES:
        tr = transition(K, tables)
        for n in ROWS:
            case = noise_case(K, n)
            out.append((tables, case) + add_noise64(tr.q_mats.detach()[case['t'][case['batch']]], case['v'], case['u']))
    return out


@functools.lru_cache(maxsize=None)
def loss_reference(K):
    """per table set and row count: dict(tables, case, row64, g64, near, gated, row32, g32) -- float64 and the same torch tail in fp32
    on the CPU"""
    out = []
    for tables in TABLES:
        tr = transition(K, tables)
        for n in ROWS:
            case = loss_case(K, n, tables)
            args = (tr.q_mats, tr.transpopse_q_onestep_mats, case['logits'], case['log_vt'], case['log_v0'], case['t'], case['batch'])
            row64, g64, near, gated = cat_loss_tail(*args)
            row32, g32, _, _ = cat_loss_tail(*args, dtype=torch.float32)
            out.append({'tables': tables, 'case': case, 'row64': row64, 'g64': g64, 'near': near, 'gated': gated, 'row32': row32.double(),
                        'g32': g32.double()})
    return out


def loss_errors(row, g, ref):
    """pooled over the entries of loss_reference(K), rows flagged `near` left out: (max |row - row64|, ||g - g64|| / ||g64||,
    max |g - g64| / max |g64|); row / g: one tensor per entry"""
    keep = [~r['near'] for r in ref]
    dr = torch.cat([(a.double() - r['row64'])[k] for a, r, k in zip(row, ref, keep)])
    dg = torch.cat([(a.double() - r['g64'])[k] for a, r, k in zip(g, ref, keep)])
    g64 = torch.cat([r['g64'][k] for r, k in zip(ref, keep)])
    return float(dr.abs().max()), float(dg.norm() / g64.norm()), float(dg.abs().max() / g64.abs().max())


def uncertainty_errors(got, logits):
    """(max over the rows with lse >= -40 of max_k |got - g64| / max_k |g64|, the rows with lse < -40 of `got`)"""
    g64, lse = uncertainty_grad(logits)
    rel = (got.double() - g64).abs().amax(dim=-1) / g64.abs().amax(dim=-1)
    return float(rel[lse >= -40.0].max()), got[lse < -40.0]
