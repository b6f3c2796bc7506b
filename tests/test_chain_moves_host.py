"""The move table of the sampler (``schedule.chain_moves``): every chain -- plain, partial, strided, resampled and their compositions --
as rows of moves with their levels, table rows, noise windows, draw indices, frames and ``step`` indices.  Every expectation below is
written out by hand from the noise-window layout DESIGN.md documents (window width W = 3T + 2; draw T - t for the move leaving level t,
T + (T - t) for its scaffold merge, 2T + 2 + t for an up-move arriving at level t, 0 the prior, 2T + 1 the initial merge; window k adds
k W).  No GPU needed."""
from moldiff_amd.schedule import chain_moves, resampling_path

N = None


def _col(rows, name):
    return [getattr(r, name) for r in rows]


def test_plain_chain_of_seven_levels():
    for scaffold in (False, True):
        ch = chain_moves(7, scaffold=scaffold)
        assert _col(ch.rows, 'kind') == ['down'] * 7
        assert _col(ch.rows, 'pos') == [0, 1, 2, 3, 4, 5, 6] and _col(ch.rows, 'pos_to') == [1, 2, 3, 4, 5, 6, 7]
        assert _col(ch.rows, 'level') == [6, 5, 4, 3, 2, 1, 0] and _col(ch.rows, 'arrive') == [5, 4, 3, 2, 1, 0, -1]
        assert _col(ch.rows, 'table') == [0, 1, 2, 3, 4, 5, 6] and _col(ch.rows, 'window') == [0] * 7
        assert _col(ch.rows, 'draw') == [1, 2, 3, 4, 5, 6, 7]                          # i + 1
        assert _col(ch.rows, 'merge_draw') == ([8, 9, 10, 11, 12, 13, 14] if scaffold else [N] * 7)   # T + 1 + i
        assert _col(ch.rows, 'frame') == [1, 2, 3, 4, 5, 6, 7] and _col(ch.rows, 'step') == [0, 1, 2, 3, 4, 5, 6]
        assert ch.prior_draw == 0 and ch.merge_draw == (15 if scaffold else N)


def test_partial_chain_started_at_step_four():
    ch = chain_moves(7, start_step=4, scaffold=True)
    assert _col(ch.rows, 'kind') == ['down'] * 4
    assert _col(ch.rows, 'level') == [3, 2, 1, 0] and _col(ch.rows, 'arrive') == [2, 1, 0, -1]
    assert _col(ch.rows, 'step') == [3, 4, 5, 6] and _col(ch.rows, 'frame') == [1, 2, 3, 4]
    assert _col(ch.rows, 'draw') == [4, 5, 6, 7] and _col(ch.rows, 'merge_draw') == [11, 12, 13, 14]
    assert _col(ch.rows, 'window') == [0] * 4
    assert ch.prior_draw is N and ch.merge_draw == 15                                  # starts from the initial merge alone: 2T + 1


def test_schedule_six_three_one_zero():
    ch = chain_moves(7, schedule=[6, 3, 1, 0], scaffold=True)
    assert _col(ch.rows, 'level') == [6, 3, 1, 0] and _col(ch.rows, 'arrive') == [3, 1, 0, -1]   # the merge levels
    assert _col(ch.rows, 'draw') == [1, 4, 6, 7]                                       # T - t
    assert _col(ch.rows, 'merge_draw') == [8, 11, 13, 14]                              # T + (T - t)
    assert _col(ch.rows, 'table') == [0, 1, 2, 3] and _col(ch.rows, 'step') == [0, 1, 2, 3] and _col(ch.rows, 'frame') == [1, 2, 3, 4]
    assert ch.prior_draw == 0 and ch.merge_draw == 15
    assert _col(chain_moves(7, schedule=[6, 3, 1, 0]).rows, 'merge_draw') == [N] * 4


# d0 d1 d2 up(3->0) d0 d1 d2 d3 d4 d5 up(6->3) d3 d4 d5 d6
KINDS = ['down'] * 3 + ['up'] + ['down'] * 6 + ['up'] + ['down'] * 4
POS = [0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 6, 3, 4, 5, 6]
POS_TO = [1, 2, 3, 0, 1, 2, 3, 4, 5, 6, 3, 4, 5, 6, 7]
WINDOWS = [0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 0]
TABLES = [0, 1, 2, (3, 0), 0, 1, 2, 3, 4, 5, (6, 3), 3, 4, 5, 6]


def test_resampled_path_of_seven_positions_in_blocks_of_three_walked_twice():
    path = resampling_path(7, 3, 2)
    ch = chain_moves(7, path=path, scaffold=True)                                       # T = 7: W = 23
    assert _col(ch.rows, 'kind') == KINDS and _col(ch.rows, 'pos') == POS and _col(ch.rows, 'pos_to') == POS_TO
    assert _col(ch.rows, 'level') == [6, 5, 4, 3, 6, 5, 4, 3, 2, 1, 0, 3, 2, 1, 0]
    assert _col(ch.rows, 'arrive') == [5, 4, 3, 6, 5, 4, 3, 2, 1, 0, 3, 2, 1, 0, -1]
    assert _col(ch.rows, 'table') == TABLES and _col(ch.rows, 'window') == WINDOWS
    # up-moves: 2T + 2 + t + W = 16 + 6 + 23 and 16 + 3 + 23; second walks: + 23
    assert _col(ch.rows, 'draw') == [1, 2, 3, 45, 24, 25, 26, 4, 5, 6, 42, 27, 28, 29, 7]
    assert _col(ch.rows, 'merge_draw') == [8, 9, 10, N, 31, 32, 33, 11, 12, 13, N, 34, 35, 36, 14]
    assert _col(ch.rows, 'frame') == list(range(1, 16))
    assert _col(ch.rows, 'step') == [0, 1, 2, N, 0, 1, 2, 3, 4, 5, N, 3, 4, 5, 6]
    assert ch.prior_draw == 0 and ch.merge_draw == 15
    draws = _col(ch.rows, 'draw') + [d for d in _col(ch.rows, 'merge_draw') if d is not N] + [0, 15]
    assert len(set(draws)) == len(draws)                                               # fresh noise on every visit


def test_resampled_path_composed_with_a_schedule_and_start_step():
    path = resampling_path(7, 3, 2)
    # T = 20 (W = 62), a partial chain from step 16 on the schedule 15 12 9 7 4 1 0: iterations are schedule positions
    ch = chain_moves(20, start_step=16, schedule=[15, 12, 9, 7, 4, 1, 0], path=path, scaffold=True)
    assert _col(ch.rows, 'kind') == KINDS and _col(ch.rows, 'table') == TABLES and _col(ch.rows, 'window') == WINDOWS
    assert _col(ch.rows, 'level') == [15, 12, 9, 7, 15, 12, 9, 7, 4, 1, 0, 7, 4, 1, 0]
    assert _col(ch.rows, 'arrive') == [12, 9, 7, 15, 12, 9, 7, 4, 1, 0, 7, 4, 1, 0, -1]
    assert _col(ch.rows, 'draw') == [5, 8, 11, 119, 67, 70, 73, 13, 16, 19, 111, 75, 78, 81, 20]
    assert _col(ch.rows, 'merge_draw') == [25, 28, 31, N, 87, 90, 93, 33, 36, 39, N, 95, 98, 101, 40]
    assert _col(ch.rows, 'step') == [0, 1, 2, N, 0, 1, 2, 3, 4, 5, N, 3, 4, 5, 6] and _col(ch.rows, 'frame') == list(range(1, 16))
    assert ch.prior_draw is N and ch.merge_draw == 41
    # without the schedule: start_step = 7 walks the levels 6 .. 0, loop iterations 13 .. 19
    ch = chain_moves(20, start_step=7, path=path, scaffold=True)
    assert _col(ch.rows, 'level') == [6, 5, 4, 3, 6, 5, 4, 3, 2, 1, 0, 3, 2, 1, 0] and _col(ch.rows, 'table') == TABLES
    assert _col(ch.rows, 'step') == [13, 14, 15, N, 13, 14, 15, 16, 17, 18, N, 16, 17, 18, 19]
    assert _col(ch.rows, 'draw') == [14, 15, 16, 110, 76, 77, 78, 17, 18, 19, 107, 79, 80, 81, 20]
    assert _col(ch.rows, 'merge_draw') == [34, 35, 36, N, 96, 97, 98, 37, 38, 39, N, 99, 100, 101, 40]
    assert ch.prior_draw is N and ch.merge_draw == 41


def test_resample_one_is_exactly_the_plain_rows():
    for kw in (dict(), dict(scaffold=True), dict(schedule=[6, 3, 1, 0], scaffold=True), dict(start_step=4, scaffold=True)):
        m = len(kw.get('schedule', range(kw.get('start_step', 7))))
        for J in (1, m - 1):
            assert chain_moves(7, path=resampling_path(m, J, 1), **kw) == chain_moves(7, **kw)
