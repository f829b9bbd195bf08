"""CPU: the launch plan of the 16-point fused kernel's last round (pinn_unit_tail_plan, jet_kernel_u16.h).

grid = min(256, ceil(N / 32)) workgroups; R = N // (16 grid) full rounds of 16-point units; the M = N - 16 grid R points
left are G = ceil(M / (4 grid)) four-point groups per workgroup: G = 1..3 one packed round (workgroup b takes the points
first_tail + 4 G b .. + 4 G - 1 below N), G = 4 ordinary units, G = 0 nothing."""

import pytest


def _grid(n):
    return min(256, -(-n // 32))


def _plan(n):
    from pinnrl_amd import _lib

    return _lib.u16_tail_plan(n, _grid(n))


def _covered(n):
    """Sorted (first, end) point ranges of the plan: full rounds (unit u of round r: workgroup u - r grid), then the tail."""
    grid = _grid(n)
    rounds, groups, first = _plan(n)
    assert first == 16 * grid * rounds
    ranges = [(0, first)] if rounds else []  # units 0 .. grid R - 1, each full: 16 u .. 16 u + 15
    if 1 <= groups <= 3:
        for b in range(grid):
            lo = first + 4 * groups * b
            hi = min(lo + 4 * groups, n)
            if lo < hi:
                ranges.append((lo, hi))
    elif groups == 4:
        u = first // 16
        while 16 * u < n:  # ordinary units first / 16 + b, b < grid
            assert u - first // 16 < grid
            ranges.append((16 * u, min(16 * u + 16, n)))
            u += 1
    return ranges


def test_every_point_once_and_the_group_rule():
    for n in list(range(1, 20_001)) + [49_729]:
        grid = _grid(n)
        rounds, groups, first = _plan(n)
        m = n - 16 * grid * rounds
        assert 0 <= m < 16 * grid and 0 <= groups <= 4, (n, rounds, groups)
        assert (groups == 0) == (m == 0), (n, m, groups)
        assert (groups == 4) == (m > 12 * grid), (n, m, groups)  # the packed round is chosen for 1 <= G <= 3 only
        if 1 <= groups <= 3:
            assert 4 * (groups - 1) * grid < m <= 4 * groups * grid, (n, m, groups)
        end = 0
        for lo, hi in _covered(n):
            assert lo == end and hi > lo, f"N={n}: range {(lo, hi)} after {end}"
            end = hi
        assert end == n, f"N={n}: covered up to {end}"


def test_headline_batch():
    assert _grid(49_729) == 256
    assert _plan(49_729) == (12, 1, 12 * 4096)


def test_small_cases_of_the_gpu_tests():
    want = {3: (1, 0, 1), 20: (1, 1, 1), 24: (1, 1, 2), 27: (1, 1, 3), 29: (1, 1, 4), 50: (2, 1, 3), 70: (3, 1, 2), 98: (4, 1, 3),
            17: (1, 1, 1), 32: (1, 2, 0), 4_900: (154, 1, 4)}
    for n, (grid, rounds, groups) in want.items():
        assert _grid(n) == grid
        assert _plan(n)[:2] == (rounds, groups), n


def test_bad_arguments_are_refused():
    from pinnrl_amd import _lib

    with pytest.raises(_lib.JetLibraryError):
        _lib.u16_tail_plan(10, 0)
    with pytest.raises(_lib.JetLibraryError):
        _lib.u16_tail_plan(-1, 4)
