"""Timestep schedules of strided sampling: which levels of the forward process the reverse chain visits.

A schedule is a strictly decreasing list of levels tau_0 > tau_1 > ... > tau_{m-1} = 0 with tau_0 = `top` (T - 1, or start_step - 1
for a partial chain).  Loop iteration j of the sampler takes the state at level tau_j, evaluates the denoiser (and the guidance)
with t = tau_j and writes the state at level tau_{j+1}; the last iteration (level 0) is the chain's ordinary t == 0 step.  The
reference has no such thing (its loop visits every level): an addition, like scaffolds.  Host code, integers only.

Resampling (RePaint's loop around replacement conditioning, another addition) makes the walk non-monotone: ``resampling_path`` lists the
moves -- down-moves between neighbouring schedule POSITIONS and up-moves back to the start of a block -- and ``draw_index`` says
which noise draw each of them uses.  ``chain_moves`` puts all of it into one table: every chain, plain, partial, strided or resampled,
is a list of ``Move`` rows that the sampler executes one after the other.
"""
import numbers
from collections import namedtuple


def make_schedule(top, num_steps):
    """Uniform schedule of `num_steps` levels from `top` down to 0: tau_j = (top (m-1-j) + (m-1)//2) // (m-1) -- the multiples of
    top / (m-1) rounded to nearest in integer arithmetic.  2 <= num_steps <= top + 1 makes the spacing >= 1, hence the levels
    distinct; num_steps = top + 1 gives top, top - 1, ..., 0."""
    for name, v in (('top', top), ('num_steps', num_steps)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f'{name} must be an int, got {v!r}')
    top, m = int(top), int(num_steps)
    if top < 1:
        raise ValueError(f'a schedule needs a top level >= 1, got {top}')
    if not 2 <= m <= top + 1:
        raise ValueError(f'num_steps {m} outside [2, {top + 1}] for a chain that starts at level {top}')
    return [(top * (m - 1 - j) + (m - 1) // 2) // (m - 1) for j in range(m)]


def check_schedule(timesteps, top):
    """Validate an explicit list of levels: ints, strictly decreasing, from `top` down to 0.  Returns it as a list of ints."""
    try:
        ts = list(timesteps)
    except TypeError:
        raise ValueError(f'timesteps must be a sequence of ints, got {timesteps!r}') from None
    for v in ts:
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f'timesteps must be ints, got {v!r}')
    ts = [int(v) for v in ts]
    if not ts:
        raise ValueError('timesteps is empty')
    if ts[0] != top:
        raise ValueError(f'timesteps must start at level {top} (T - 1, or start_step - 1), got {ts[0]}')
    if ts[-1] != 0:
        raise ValueError(f'timesteps must end at level 0, got {ts[-1]}')
    if any(b >= a for a, b in zip(ts, ts[1:])):
        raise ValueError('timesteps must be strictly decreasing')
    return ts


def resolve_schedule(top, num_steps=None, timesteps=None):
    """The schedule the keywords of ``MolDiff.sample`` ask for, or None when neither is given (the full chain's own code path)."""
    if num_steps is not None and timesteps is not None:
        raise ValueError('give num_steps or timesteps, not both')
    if num_steps is not None:
        return make_schedule(top, num_steps)
    if timesteps is not None:
        return check_schedule(timesteps, top)
    return None


def pairs(schedule):
    """(t, s) of every iteration: (tau_j, tau_{j+1}), and (0, -1) for the last one (nothing below level 0)."""
    return list(zip(schedule, list(schedule[1:]) + [-1]))


# ---- resampling: a path over schedule positions that walks every block of levels several times ---------------------------------------

def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise ValueError(f'{name} must be an int, got {v!r}')
    return int(v)


def resampling_path(m, jump_length, resample):
    """The moves of a resampling chain over `m` schedule positions p = 0..m-1 (position p is level tau_p of a schedule, or level
    top - p of the full chain; position m-1 is level 0).

    Block boundaries are the multiples of `jump_length` and, last, position m-1 (the final block is shorter when m-1 is no multiple).
    Every block [a, b] is walked a -> b `resample` times: one walk is the down-moves ('down', p), p = a..b-1 (the state at position p
    goes to position p + 1); between two walks comes one up-move ('up', b, a), the forward diffusion from position b back to position
    a.  After the last block comes the chain's ordinary final move ('down', m-1): level 0 to x_0, once.
    Denoiser evaluations: resample (m-1) + 1; up-moves: (resample-1) ceil((m-1) / jump_length); resample = 1 gives the m down-moves of
    the plain chain."""
    m, J, R = _int('m', m), _int('jump_length', jump_length), _int('resample', resample)
    if m < 2:
        raise ValueError(f'a path needs at least 2 schedule positions, got {m}')
    if R < 1:
        raise ValueError(f'resample must be >= 1, got {R}')
    if not 1 <= J <= m - 1:
        raise ValueError(f'jump_length {J} outside [1, {m - 1}] for a chain of {m} positions')
    path = []
    for a in range(0, m - 1, J):
        b = min(a + J, m - 1)
        for k in range(R):
            if k:
                path.append(('up', b, a))
            path.extend(('down', p) for p in range(a, b))
    path.append(('down', m - 1))
    return path


def resolve_path(m, jump_length=None, resample=None):
    """The path the keywords of ``MolDiff.sample`` ask for, or None when neither is given (the chain's own loop).  The two come
    together: one without the other raises (resample = 1 with a jump_length is allowed and is the plain chain)."""
    if jump_length is None and resample is None:
        return None
    if jump_length is None or resample is None:
        raise ValueError('resample and jump_length come together: give both or neither')
    return resampling_path(m, jump_length, resample)


def path_windows(path):
    """The noise window of every move of a path: the k-th walk of a block (k = 0, 1, ..) uses window k, and so does the up-move that
    opens it.  Read off the path itself: a down-move at position p is in the walk numbered by the earlier down-moves at p, an up-move
    (b, a) opens the walk numbered 1 + the earlier up-moves (b, a).  The final move is made once: window 0."""
    seen, out = {}, []
    for mv in path:
        k = seen.get(mv, 0)
        seen[mv] = k + 1
        out.append(k + 1 if mv[0] == 'up' else k)
    return out


def window_width(T):
    """W = 3T + 2 draw indices per window: 0 the prior, T - t the move leaving level t, T + (T - t) its scaffold merge, 2T + 1 the initial
    merge, 2T + 2 + t an up-move arriving at level t (t < T, so the last index used is 3T + 1)."""
    return 3 * int(T) + 2


def draw_index(T, kind, level=None, window=0):
    """Philox draw index of one piece of a chain's noise.  kind: 'prior' | 'init_merge' (no level) | 'down' (the move LEAVING `level`) |
    'merge' (the scaffold merge after the move leaving `level`) | 'up' (an up-move ARRIVING at `level`).  Window 0 is what the plain,
    strided and scaffold chains use; the k-th walk of a resampling block adds k W."""
    T, window = int(T), int(window)
    if kind in ('prior', 'init_merge'):
        base = 0 if kind == 'prior' else 2 * T + 1
    else:
        t = int(level)
        if not 0 <= t < T:
            raise ValueError(f'level {level} outside [0, {T})')
        base = {'down': T - t, 'merge': T + (T - t), 'up': 2 * T + 2 + t}[kind]
    if window < 0:
        raise ValueError(f'window {window} < 0')
    return base + window * window_width(T)


def check_draw_range(T, resample):
    """`draw` is an int32 that the Philox key takes as uint32: every index of `resample` windows must stay below 2^31."""
    if int(resample) * window_width(T) >= 2 ** 31:
        raise ValueError(f'resample {resample} x {window_width(T)} draw indices per window does not fit the 31-bit draw index')


Move = namedtuple('Move', 'kind pos pos_to level arrive table window draw merge_draw frame step')
Move.__doc__ = """One row of a chain's move table.  kind: 'down' | 'up'; pos -> pos_to: the schedule positions left and arrived at (a
down-move: p -> p + 1); level -> arrive: their levels (arrive = -1 below level 0); table: the jump-table row of a down-move (its
position), the forward-table key (b, a) of an up-move; window: the noise window; draw: the draw index of the move; merge_draw: that
of the scaffold merge after a down-move (None without a scaffold and after an up-move; the merge at arrive = -1 copies x_0 and
consumes no noise); frame: the trajectory frame written; step: the loop iteration i of ``step(i)`` (None for an up-move)."""

Chain = namedtuple('Chain', 'rows prior_draw merge_draw')
Chain.__doc__ = """rows: the moves in order; prior_draw / merge_draw: the draw indices of the initial state -- the prior draw (None for a
partial chain, which starts from the scaffold molecule) and the merge of the scaffold into it (None without a scaffold)."""


def _rows(T, levels, path, scaffold, step0):
    """The rows of `path` over positions of levels `levels`; step0: the loop iteration of position 0."""
    m, rows = len(levels), []
    for k, (mv, w) in enumerate(zip(path, path_windows(path))):
        if mv[0] == 'up':
            b, a = mv[1:]
            rows.append(Move('up', b, a, levels[b], levels[a], (b, a), w, draw_index(T, 'up', levels[a], w), None, k + 1, None))
        else:
            p, t = mv[1], levels[mv[1]]
            rows.append(Move('down', p, p + 1, t, levels[p + 1] if p + 1 < m else -1, p, w, draw_index(T, 'down', t, w),
                             draw_index(T, 'merge', t, w) if scaffold else None, k + 1, step0 + p))
    return rows


def chain_moves(T, start_step=None, schedule=None, path=None, scaffold=False):
    """The whole chain as a ``Chain`` of ``Move`` rows.  schedule: the levels of ``resolve_schedule`` (None: every level from the top,
    T - 1 or start_step - 1, down to 0); path: the moves of ``resolve_path`` over their positions (None: the down-moves 0..m-1, the
    plain chain, window 0).  Loop iterations count schedule positions under a schedule, and levels from T - 1 without one: ``step(i)``
    of an unscheduled partial chain takes i = T - start_step .. T - 1.  This and ``draw_index`` are all that know how a chain's noise
    is laid out."""
    T = int(T)
    top = (T if start_step is None else int(start_step)) - 1
    levels = list(schedule) if schedule is not None else list(range(top, -1, -1))
    if path is None:
        path = [('down', p) for p in range(len(levels))]
    rows = _rows(T, levels, path, scaffold, 0 if schedule is not None else T - 1 - top)
    init_merge = draw_index(T, 'init_merge') if scaffold or start_step is not None else None
    return Chain(rows, None if start_step is not None else draw_index(T, 'prior'), init_merge)


def path_draws(path, levels, T, scaffold=False, partial=False):
    """The draw indices a chain over `path` asks for, in order: a projection of its move table.  levels[p]: the level of position p.
    scaffold: a merge follows every down-move and the prior draw (the one below level 0 asks for no noise); partial (start_step): the
    chain starts from the initial merge alone."""
    out = [draw_index(T, 'init_merge')] if partial else [draw_index(T, 'prior')] + ([draw_index(T, 'init_merge')] if scaffold else [])
    for r in _rows(T, levels, path, scaffold, 0):
        out.append(r.draw)
        if r.merge_draw is not None and r.arrive >= 0:
            out.append(r.merge_draw)
    return out
