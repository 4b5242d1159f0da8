"""The launch constants of the projection kernels (ProjLaunch, ltm_kernels_common.h) are computed once per launch on the host and passed as a
kernel argument.  They must be, bit for bit, what the kernels computed per thread before: the expressions below are those expressions, evaluated in
numpy float32 (IEEE binary32, one rounding per operation, correctly rounded division and square root -- the same arithmetic on both sides).  And the
workgroup -> (map tile, keyframe) mapping, now shifts and one multiply-high, must be the mapping of the two divisions it replaces.  No device needed."""
import numpy as np
import pytest

VFOVS = (50.0, 26.9, 90.0)
HFOV = 360.0
ALPHAS = (2.5, 2.0, 1.5, 3.0, 1.0) + tuple(float(np.float32(0.95 * a)) for a in (2.5, 2.0, 1.5))
F = np.float32


def _b2l_cases():
    c, s = np.cos(0.3), np.sin(0.3)
    T = np.eye(4)
    T[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(0.05), -np.sin(0.05)], [0, np.sin(0.05), np.cos(0.05)]])
    T[:3, 3] = (0.81, -0.27, 1.93)
    return {"identity": None, "lever": T}


def _roundf(x):
    """C roundf: half away from zero"""
    x = F(x)
    return F(np.copysign(np.floor(np.abs(x) + F(0.5)), x)) if np.abs(x) < F(2 ** 23) else x


def expected_constants(ltm, vfov, hfov, alpha, b2l):
    """the device expressions of the parent commit (make_geom, k_vote_map_cull, k_map_rimg_blockmin, cull_candidates, cull_min_range, geom_for)"""
    vfov, hfov, alpha = F(vfov), F(hfov), F(alpha)
    rows, cols = int(_roundf(vfov * alpha)), int(_roundf(hfov * alpha))
    frows, fcols = F(rows), F(cols)
    el_fit = ltm.load_library().ltm_debug_elevation_fit(float(vfov), (ltm.C.c_float * 4)(), ltm.C.byref(ltm.C.c_double())) == 1
    ppd = max(frows / vfov, fcols / hfov)
    eps = max(F(1.0e-3), F(3.0e-4 if el_fit else 6.0e-4) * ppd)
    f = {"half_v": vfov / F(2.0), "half_h": hfov / F(2.0), "inv_v": F(1.0) / vfov, "inv_h": F(1.0) / hfov, "frows": frows, "fcols": fcols,
         "row_max": F(rows - 1), "col_max": F(cols - 1),
         "row_scale": frows * (F(57.29577951308232) / vfov), "col_scale": fcols * (F(57.29577951308232) / hfov),
         "row_bias": F(0.5) * frows + F(0.5) - eps, "col_bias": F(0.5) * fcols + F(0.5) - eps,
         "certain_lim": F(1.0) - F(2.0) * eps, "eps": eps}
    if b2l is None:
        f["rmin2"] = F(0.0)
    else:
        tx, ty, tz = F(b2l[0, 3]), F(b2l[1, 3]), F(b2l[2, 3])
        rmin = F(0.125) * np.sqrt(tx * tx + ty * ty + tz * tz) + F(1.0e-6)
        f["rmin2"] = rmin * rmin
    u = {"rows": rows, "cols": cols, "npx": rows * cols, "steep_clamps": int(vfov < F(88.0)), "packable": int(rows < 511 and cols <= 2048), "el_fit": int(el_fit)}
    return f, u


@pytest.mark.parametrize("b2l_name", ["identity", "lever"])
@pytest.mark.parametrize("vfov", VFOVS)
def test_host_constants_equal_the_device_expressions_bit_for_bit(ltm, vfov, b2l_name):
    b2l = _b2l_cases()[b2l_name]
    for alpha in ALPHAS:
        got_f, got_u, _, _ = ltm.proj_launch(vfov, HFOV, alpha, b2l, map_points=3 * 4096 + 5, n_keyframes=9)
        want_f, want_u = expected_constants(ltm, vfov, HFOV, alpha, b2l)
        for k, v in want_f.items():
            assert F(got_f[k]).view(np.uint32) == F(v).view(np.uint32), f"{k} at vfov {vfov} alpha {alpha} {b2l_name}: {got_f[k]!r} vs {v!r}"
        for k, v in want_u.items():
            assert got_u[k] == v, f"{k} at vfov {vfov} alpha {alpha} {b2l_name}: {got_u[k]} vs {v}"
        # (frows - 1 and cols - 1 as the clamp bounds of cull_candidates: the same numbers as row_max / col_max)
        assert F(want_f["frows"] - F(1.0)).view(np.uint32) == F(got_f["row_max"]).view(np.uint32)
        assert F(want_f["fcols"] - F(1.0)).view(np.uint32) == F(got_f["col_max"]).view(np.uint32)
    assert got_u["n_tiles"] == 4 and got_u["n_tg"] == 1


def old_tile_kf(b, n_tiles, nb, kfg=8):
    """tile_kf_of_block of the parent commit: two runtime divisions"""
    b = b.astype(np.uint64)
    x, r = b & 7, b >> 3
    n_tg = (n_tiles + 7) >> 3
    kfl, q = r % kfg, r // kfg
    tg, kg = q % n_tg, q // n_tg
    tile, kf = tg * 8 + x, kg * kfg + kfl
    valid = (tile < n_tiles) & (kf < nb)
    return np.where(valid, tile, 0xffffffff).astype(np.uint32), np.where(valid, kf, 0xffffffff).astype(np.uint32), valid


@pytest.mark.parametrize("n_tiles", [1, 7, 8, 9, 15, 16, 17, 1668, 11000])
def test_tile_mapping_is_the_old_mapping_and_hits_every_pair_once(ltm, n_tiles):
    for nb in (1, 7, 8, 9, 500, 512):
        M = n_tiles * 4096 - (n_tiles % 3)          # the last tile full or partial
        _, u, _, _ = ltm.proj_launch(50.0, HFOV, 2.5, None, map_points=M, n_keyframes=nb)
        assert u["n_tiles"] == n_tiles
        grid = u["grid"]
        assert grid == ((n_tiles + 7) // 8) * 8 * 8 * ((nb + 7) // 8)
        _, _, tile, kf = ltm.proj_launch(50.0, HFOV, 2.5, None, map_points=M, n_keyframes=nb, first_block=0, n_blocks=grid)
        w_tile, w_kf, valid = old_tile_kf(np.arange(grid), n_tiles, nb)
        assert (tile == w_tile).all() and (kf == w_kf).all(), f"n_tiles {n_tiles} nb {nb}"
        pair = tile[valid].astype(np.uint64) * nb + kf[valid]
        assert valid.sum() == n_tiles * nb and np.unique(pair).size == n_tiles * nb, "every (tile, keyframe) exactly once"


@pytest.mark.parametrize("n_tiles", [1, 3, 8, 9, 1668, 11000, 65537, (1 << 20) - 1])
def test_tile_mapping_quotient_is_exact_up_to_the_last_block_index(ltm, n_tiles):
    """the multiply-high quotient must be floor((b >> 6) / n_tg) for every b < 2^32, not only inside the grid"""
    rng = np.random.default_rng(n_tiles)
    nb = 0xfffffffe                                                  # every keyframe index valid: the comparison sees the quotient itself
    M = n_tiles * 4096
    n_tg = (n_tiles + 7) // 8
    runs = [0, (1 << 32) - 4096, (1 << 31) - 2048] + [int(v) for v in rng.integers(0, (1 << 32) - 4096, 24)]
    runs += [min(max(k * n_tg * 64 - 2048, 0), (1 << 32) - 4096) for k in (1, 2, 3, (1 << 26) // n_tg - 1, (1 << 26) // n_tg)]      # around multiples of the divisor
    for first in runs:
        _, _, tile, kf = ltm.proj_launch(50.0, HFOV, 2.5, None, map_points=M, n_keyframes=nb, first_block=first, n_blocks=4096)
        w_tile, w_kf, _ = old_tile_kf(np.arange(first, first + 4096, dtype=np.uint64), n_tiles, nb)
        assert (tile == w_tile).all() and (kf == w_kf).all(), f"n_tiles {n_tiles} blocks from {first}"
