"""One workgroup of the range-culled vote kernel takes a run of T consecutive map tiles for one keyframe (RunLaunch, ltm_kernels_common.h; context switch
LTM_VOTE_TILE_RUN).  The workgroup -> (run, keyframe) mapping, read through ltm_debug_vote_run_launch, must cover every (tile, keyframe) pair exactly
once and nothing else for every run length, be the one-tile mapping of ltm_debug_proj_launch at T = 1, and its multiply-high quotient must be exact for
every block index below 2^32.  No device needed."""
import numpy as np
import pytest

RUN_LENGTHS = (1, 2, 3, 4, 8)
KEYFRAMES = (1, 7, 8, 9, 500)
IDLE = 0xffffffff


def _tile_counts(T):
    return sorted({n for n in (1, T - 1, T, T + 1, 8 * T - 1, 8 * T, 8 * T + 1, 1668) if n >= 1})


def _reference(b, n_runs, nb):
    """the mapping with its two divisions: b = ((kg * n_rg + rg) * 8 + kfl) * 8 + x -> run rg * 8 + x, keyframe kg * 8 + kfl"""
    b = b.astype(np.uint64)
    x, kfl, q = b & 7, (b >> 3) & 7, b >> 6
    n_rg = (n_runs + 7) // 8
    rg, kg = q % n_rg, q // n_rg
    run, kf = rg * 8 + x, kg * 8 + kfl
    valid = (run < n_runs) & (kf < nb)
    return np.where(valid, run, IDLE).astype(np.uint32), np.where(valid, kf, IDLE).astype(np.uint32), valid


@pytest.mark.parametrize("T", RUN_LENGTHS)
def test_every_tile_keyframe_pair_is_hit_exactly_once_and_nothing_else(ltm, T):
    for n_tiles in _tile_counts(T):
        n_runs = -(-n_tiles // T)
        for nb in KEYFRAMES:
            M = n_tiles * 4096 - (n_tiles % 3)          # the last tile full or partial
            _, _, run_len, grid = ltm.vote_run_launch(M, nb, T)
            assert run_len == T
            assert grid == ((n_runs + 7) // 8) * 64 * ((nb + 7) // 8), f"T {T} n_tiles {n_tiles} nb {nb}"
            run, kf, _, _ = ltm.vote_run_launch(M, nb, T, first_block=0, n_blocks=grid)
            w_run, w_kf, valid = _reference(np.arange(grid), n_runs, nb)
            what = f"T {T} n_tiles {n_tiles} nb {nb}"
            assert (run == w_run).all() and (kf == w_kf).all(), what
            assert ((run == IDLE) == (kf == IDLE)).all(), what
            # expand the runs into their tiles, as the kernel does: [r T, min((r + 1) T, n_tiles))
            hits = np.zeros((n_tiles, nb), dtype=np.int64)
            r, k = run[valid].astype(np.int64), kf[valid].astype(np.int64)
            assert (r < n_runs).all() and (k < nb).all(), f"{what}: an invalid pair is hit"
            for t in range(T):
                tile = r * T + t
                ok = tile < n_tiles
                np.add.at(hits, (tile[ok], k[ok]), 1)
            assert (r * T < n_tiles).all(), f"{what}: an empty run is launched"
            assert (hits == 1).all(), f"{what}: {(hits != 1).sum()} (tile, keyframe) pairs not hit exactly once"
            # beyond the grid nothing is valid
            run, kf, _, _ = ltm.vote_run_launch(M, nb, T, first_block=grid, n_blocks=128)
            assert (run == IDLE).all() and (kf == IDLE).all(), f"{what}: work beyond the grid"


@pytest.mark.parametrize("n_tiles", [1, 7, 8, 9, 17, 1668])
def test_run_length_one_is_the_tile_mapping(ltm, n_tiles):
    for nb in KEYFRAMES:
        M = n_tiles * 4096 - (n_tiles % 3)
        _, u, _, _ = ltm.proj_launch(50.0, 360.0, 2.5, None, map_points=M, n_keyframes=nb)
        _, _, run_len, grid = ltm.vote_run_launch(M, nb, 1)
        assert run_len == 1 and grid == u["grid"]
        _, _, tile, kf = ltm.proj_launch(50.0, 360.0, 2.5, None, map_points=M, n_keyframes=nb, first_block=0, n_blocks=grid + 64)
        run, rkf, _, _ = ltm.vote_run_launch(M, nb, 1, first_block=0, n_blocks=grid + 64)
        assert (run == tile).all() and (rkf == kf).all(), f"n_tiles {n_tiles} nb {nb}"


@pytest.mark.parametrize("T", RUN_LENGTHS)
def test_quotient_is_exact_up_to_the_last_block_index(ltm, T):
    """the multiply-high quotient must be floor((b >> 6) / n_rg) for every b < 2^32, not only inside the grid"""
    nb = 0xfffffffe                                                  # every keyframe index valid: the comparison sees the quotient itself
    for n_tiles in _tile_counts(T) + [11000, 65537, (1 << 20) - 1]:
        rng = np.random.default_rng(n_tiles * 17 + T)
        n_runs = -(-n_tiles // T)
        n_rg = (n_runs + 7) // 8
        firsts = [0, (1 << 32) - 4096, (1 << 31) - 2048] + [int(v) for v in rng.integers(0, (1 << 32) - 4096, 8)]
        firsts += [min(max(k * n_rg * 64 - 2048, 0), (1 << 32) - 4096) for k in (1, 2, 3, (1 << 26) // n_rg - 1, (1 << 26) // n_rg)]      # around multiples of the divisor
        for first in firsts:
            run, kf, _, _ = ltm.vote_run_launch(n_tiles * 4096, nb, T, first_block=first, n_blocks=4096)
            w_run, w_kf, _ = _reference(np.arange(first, first + 4096, dtype=np.uint64), n_runs, nb)
            assert (run == w_run).all() and (kf == w_kf).all(), f"T {T} n_tiles {n_tiles} blocks from {first}"
        assert max(firsts) + 4095 == (1 << 32) - 1, "the last block index below 2^32 is among the checked ones"


def test_run_length_is_clamped(ltm):
    assert ltm.vote_run_launch(10 * 4096, 3, 64)[2] == 16
    with pytest.raises(ltm.LtmError):
        ltm.vote_run_launch(10 * 4096, 3, 0)
