"""Timestep schedules of strided sampling: which levels of the forward process the reverse chain visits.

A schedule is a strictly decreasing list of levels tau_0 > tau_1 > ... > tau_{m-1} = 0 with tau_0 = `top` (T - 1, or start_step - 1
for a partial chain).  Loop iteration j of the sampler takes the state at level tau_j, evaluates the denoiser (and the guidance)
with t = tau_j and writes the state at level tau_{j+1}; the last iteration (level 0) is the chain's ordinary t == 0 step.  The
reference has no such thing (its loop visits every level): an addition, like scaffolds.  Host code, integers only.
"""
import numbers


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
