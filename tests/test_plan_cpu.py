"""Which engine an LP gets (ellp_plan.inc: plan_engine), asked through ellp_engine_plan — no device needed.

The expectations below are written by hand from the documented defaults (README.md, include/ellp_hip.h);
none is produced by calling the function.  Each row names the fields it pins; CASES is also the grid over which the plan
was compared with the engines the parent commit creates (profiles/plan_refactor_modes.txt)."""
import numpy as np
import pytest

from ellp_amd import _engine as E
from helpers import unit_basis_problem

P, D = E.ENGINE_PRIMAL, E.ENGINE_DUAL
DENSE, MAXVIOL, SE, NOCERT, BFLIP = (E.FLAG_DENSE_PRICING, E.FLAG_DUAL_MAX_VIOLATION, E.FLAG_PRIMAL_STEEPEST_EDGE,
                                     E.FLAG_NO_CERTIFY, E.FLAG_DUAL_BOUND_FLIPPING)
ENV_VARS = ("ELLP_MID_AUTO_MAX", "ELLP_ILL_TOL", "ELLP_DRIFT_EVERY", "ELLP_DRIFT_TOL", "ELLP_NO_UNIT_COLUMNS", "ELLP_SMALL_STAMPS",
            "ELLP_SMALL_NT", "ELLP_NO_HYBRID", "ELLP_GUARD_ABS", "ELLP_EXACT_K", "ELLP_DUAL_FOLD_OFF", "ELLP_SE_BTRAN")

# the loops, as the fields that tell them apart
K_SMALL = dict(small=1, mid=0, hybrid=0, cert_large=0, exact_large_always=0, lagged=0, dual_fused=0)
K_MID = dict(small=1, mid=1, hybrid=0, cert_large=0, exact_large_always=0, lagged=0, dual_fused=0)
HYBRID = dict(small=0, mid=0, hybrid=1, cert_large=0, exact_large_always=0, lagged=0, dual_fused=0, guard_abs=1e-7, exact_K=8)
THREE = dict(small=0, mid=0, hybrid=0, cert_large=0, exact_large_always=0, lagged=0, dual_fused=0, guard_abs=0.0)  # plain, three launches
TWO_P = dict(small=0, mid=0, hybrid=0, cert_large=0, exact_large_always=0, lagged=1, dual_fused=0)  # primal, two launches
TWO_D = dict(small=0, mid=0, hybrid=0, cert_large=0, exact_large_always=0, lagged=0, dual_fused=1)  # dual, fused
CERT_P = dict(TWO_P, cert_large=1, guard_abs=1e-7)
CERT_D = dict(TWO_D, cert_large=1, guard_abs=1e-7)
EXACT_LARGE = dict(small=0, mid=0, hybrid=0, cert_large=0, exact_large_always=1, lagged=0, dual_fused=0, guard_abs=0.0)


def row(kind, m, nN, want, env=None, **opts):
    return (kind, m, nN, opts, env or {}, want)


CASES = [
    # ---- rows: 64 | 65 (one wave), 128 | 129 (k_small's limit), default options, both kinds
    row(P, 3, 5, dict(K_SMALL, ld=16, small_nt=64, ill_tol=1e-3, upd_rows=1, upd_blocks=3, priceT=1, cpb=1, nblocks=5, nbs=5, seg=20,
                      btran_rows=8, btran_tiles=1, ftran_blocks=1, bl_splits=8, upd_stage=1, drift_every=0, drift_tol=1e-10,
                      refactor_period=0, unit_table=1, stamps=0, pp_P=0, se=0, dual_bflip=0, dual_maxviol=0, price_nt=0, price_wave=0)),
    row(D, 3, 5, dict(K_SMALL, small_nt=64)),
    row(P, 64, 100, dict(K_SMALL, small_nt=64)),
    row(P, 65, 100, dict(K_SMALL, small_nt=128)),
    row(P, 60, 2049, dict(K_SMALL, small_nt=256)),  # many columns: the widest workgroup
    row(P, 128, 200, dict(K_SMALL, ld=128, small_nt=128, mid_lds=0)),
    row(D, 128, 200, dict(K_SMALL, small_nt=128)),
    row(P, 129, 200, dict(HYBRID, ld=144, mid_nt=256, ldn=208, small_lds=0, ill_tol=1e-3)),
    row(D, 129, 200, dict(HYBRID, mid_nt=256, ldn=208)),
    # ---- 255 | 256: rows per block of the rebuild, k_mid's workgroup
    row(P, 255, 300, dict(HYBRID, upd_rows=1, upd2_rows=1, upd_blocks=255, mid_nt=256)),
    row(P, 256, 300, dict(HYBRID, upd_rows=2, upd2_rows=2, upd_blocks=128, upd2_blocks=128, mid_nt=256)),
    row(P, 257, 300, dict(HYBRID, mid_nt=512)),
    # ---- 383 | 384: two launches per iteration (where the hybrid is off)
    row(P, 383, 500, HYBRID),
    row(P, 384, 500, HYBRID),
    row(P, 383, 500, THREE, flags=NOCERT),
    row(P, 384, 500, TWO_P, flags=NOCERT),
    row(D, 383, 500, THREE, flags=NOCERT),
    row(D, 384, 500, dict(TWO_D, dual_fold=0), flags=NOCERT),  # ill_tol > 0 up to 512 rows: the closing work is not folded
    # ---- 512 | 513: reactive maintenance, BTRAN tiles, k_mid's workgroup
    row(P, 512, 600, dict(HYBRID, ill_tol=1e-3, btran_rows=8, btran_tiles=64, mid_nt=512, priceT=1)),
    row(P, 513, 600, dict(HYBRID, ill_tol=0.0, btran_rows=9, btran_tiles=57, mid_nt=1024, ld=528, priceT=2)),
    row(D, 512, 600, dict(TWO_D, ill_tol=1e-3, dual_fold=0), flags=NOCERT),
    row(D, 513, 600, dict(TWO_D, ill_tol=0.0, dual_fold=1), flags=NOCERT),
    # ---- 1,024 | 1,025: k_mid's limit
    row(P, 1023, 1200, dict(HYBRID, upd_rows=2)),
    row(P, 1024, 1200, dict(HYBRID, upd_rows=4, upd_blocks=256, ld=1024, priceT=2)),
    row(P, 1025, 1200, dict(CERT_P, ld=1040, priceT=4, mid_lds=0, mid_nt=0, ldn=0)),
    row(D, 1024, 1200, HYBRID),
    row(D, 1025, 1200, dict(CERT_D, dual_fold=1)),
    row(P, 1025, 2, CERT_P),
    row(D, 1025, 2, dict(CERT_D, dual_fold=1)),
    row(P, 1024, 1200, dict(K_MID, mid_nt=1024, ldn=1200), pipeline=3),
    row(P, 1025, 1200, EXACT_LARGE, pipeline=3),
    row(D, 1024, 1200, K_MID, pipeline=3),
    row(D, 1025, 1200, EXACT_LARGE, pipeline=3),
    row(P, 1025, 1200, dict(TWO_P, guard_abs=0.0), flags=NOCERT),
    # ---- 2,047 | 2,048 (FTRAN blocks), 2,304 | 2,305 (splits of the rebuild's first GEMM)
    row(P, 2047, 100, dict(CERT_P, ftran_blocks=512, ld=2048, priceT=4)),
    row(P, 2048, 100, dict(CERT_P, ftran_blocks=512)),
    row(P, 2049, 100, dict(CERT_P, ftran_blocks=512, ld=2064, priceT=8)),
    row(P, 2304, 100, dict(CERT_P, bl_splits=8)),
    row(P, 2305, 100, dict(CERT_P, bl_splits=7)),
    # ---- 3,071 | 3,072: rows per block of k_update2; 3,119 | 3,120: its staged fold inputs leave LDS
    row(P, 3071, 100, dict(CERT_P, upd2_rows=4, upd2_blocks=768, upd_rows=4)),
    row(P, 3072, 100, dict(CERT_P, upd2_rows=8, upd2_blocks=384, upd_rows=4, upd_blocks=768)),
    row(D, 3072, 100, dict(CERT_D, upd2_rows=8)),
    row(P, 3119, 100, dict(CERT_P, upd_stage=1, upd_lds=8 * 49 + 13 * 3119 + 16)),
    row(P, 3120, 100, dict(CERT_P, upd_stage=0, upd_lds=8 * 49 + 16)),
    # ---- 4,096 | 4,097 (ld 4,096 | 4,112): the fused dual, wave pricing under the two-launch pipeline, steepest edge's v
    row(D, 4096, 100, dict(CERT_D, ld=4096, dual_fold=1, priceT=8)),
    row(D, 4097, 100, dict(THREE, ld=4112, cert_large=1, guard_abs=1e-7, dual_fold=0, priceT=16)),
    row(P, 4096, 4200, dict(CERT_P, cpb=5, price_nt=0, price_wave=1)),
    row(P, 4097, 4200, dict(CERT_P, cpb=5, price_nt=0, price_wave=0)),
    row(P, 4096, 4200, dict(THREE, se=1, se_vpart=1, upd2_rows=4, price_wave=1, ill_tol=1e-3), flags=SE),
    row(P, 4097, 4200, dict(THREE, se=1, se_vpart=0, upd2_rows=8, price_wave=1, ill_tol=1e-3), flags=SE),
    # ---- 8,192: the widest pricing tile (8,193: test_refusals)
    row(P, 8192, 10, dict(CERT_P, ld=8192, priceT=16, btran_rows=128, btran_tiles=64, bl_splits=2)),
    row(D, 8192, 10, dict(THREE, cert_large=1, guard_abs=1e-7)),
    # ---- |N| = 0, 1
    row(P, 3, 0, dict(K_SMALL, cpb=1, nblocks=1, seg=4, unit_table=0)),
    row(P, 200, 0, dict(THREE, unit_table=0, ldn=0)),
    row(D, 200, 0, THREE),
    row(P, 2000, 0, THREE),
    row(D, 2000, 0, THREE),
    row(P, 2000, 0, EXACT_LARGE | dict(exact_large_always=0), pipeline=3),
    row(P, 200, 1, dict(HYBRID, cpb=1, nblocks=1, ldn=16, unit_table=1)),
    row(D, 200, 1, HYBRID),
    # ---- |N| = 4,096 | 4,097 (columns per pricing block 4 | 5) with ld = 512 and below it
    row(P, 512, 4096, dict(HYBRID, cpb=4, nblocks=1024, nbs=1024, seg=10240, price_wave=0, ftran_lds=8 * 1024 + 16)),
    row(P, 512, 4097, dict(HYBRID, cpb=5, nblocks=820, nbs=820, seg=9840, price_wave=1)),
    row(P, 496, 4097, dict(HYBRID, cpb=5, price_wave=0)),
    # ---- 8 ld |N| = 160e6 at ld = 1,024: streaming loads, twice the blocks
    row(P, 1024, 19531, dict(HYBRID, price_nt=0, cpb=20, nblocks=977, price_wave=1)),
    row(P, 1024, 19532, dict(HYBRID, price_nt=1, cpb=10, nblocks=1954, price_wave=0)),
    # ---- an |N| k_mid's LDS layout does not take (more than 4,096 chunks of 64 columns)
    row(P, 200, 262144, dict(HYBRID, cpb=64, nblocks=4096, price_nt=1)),
    row(P, 200, 262145, dict(THREE, mid_lds=0, cpb=64, nblocks=4097)),
    row(D, 200, 262145, dict(THREE, mid_lds=0)),
    row(P, 200, 262145, dict(THREE, mid_lds=0), pipeline=3),
    # ---- pipelines 0 to 3 at 100, 200 and 2,000 rows
    row(P, 100, 300, K_SMALL, pipeline=0),
    row(P, 100, 300, THREE, pipeline=1),
    row(P, 100, 300, TWO_P, pipeline=2),
    row(P, 100, 300, K_SMALL, pipeline=3),
    row(D, 100, 300, THREE, pipeline=1),
    row(D, 100, 300, dict(TWO_D, dual_fold=0), pipeline=2),
    row(D, 100, 300, K_SMALL, pipeline=3),
    row(P, 200, 300, THREE, pipeline=1),
    row(P, 200, 300, TWO_P, pipeline=2),
    row(P, 200, 300, dict(K_MID, mid_nt=256, ldn=304), pipeline=3),
    row(D, 200, 300, THREE, pipeline=1),
    row(D, 200, 300, TWO_D, pipeline=2),
    row(D, 200, 300, dict(K_MID, mid_nt=256, ldn=304), pipeline=3),
    row(P, 2000, 300, THREE, pipeline=1),
    row(P, 2000, 300, dict(TWO_P, guard_abs=0.0), pipeline=2),
    row(D, 2000, 300, THREE, pipeline=1),
    row(D, 2000, 300, dict(TWO_D, cert_large=0, dual_fold=1), pipeline=2),
    row(D, 5000, 300, THREE, pipeline=2),  # ld > 4,096: no fused dual on request either
    # ---- the two flags
    row(P, 100, 300, K_SMALL, flags=NOCERT),
    row(P, 200, 300, THREE, flags=NOCERT),
    row(D, 200, 300, THREE, flags=NOCERT),
    row(P, 2000, 300, dict(TWO_P, guard_abs=0.0), flags=NOCERT),
    row(P, 200, 300, dict(HYBRID, unit_table=0), flags=DENSE),
    row(D, 200, 300, dict(HYBRID, unit_table=0), flags=DENSE),
    row(P, 200, 300, dict(THREE, se=1, unit_table=1), flags=DENSE | SE),  # steepest edge needs the table for its permutation test
    # ---- steepest edge (primal; a dual engine ignores the flag)
    row(P, 17, 30, dict(THREE, se=1, se_vpart=1, ill_tol=1e-3, unit_table=1), flags=SE),
    row(P, 200, 300, dict(THREE, se=1, se_vpart=1), flags=SE),
    row(P, 2000, 300, dict(THREE, se=1, se_vpart=1, ill_tol=1e-3), flags=SE),
    row(P, 3500, 300, dict(THREE, se=1, se_vpart=1, upd2_rows=4), flags=SE),
    row(P, 200, 300, dict(THREE, se=1), flags=SE, pipeline=1),
    row(P, 200, 0, dict(THREE, se=0, ill_tol=1e-3), flags=SE),
    row(D, 200, 300, dict(HYBRID, se=0), flags=SE),
    row(D, 2000, 300, dict(CERT_D, se=0, ill_tol=0.0), flags=SE),
    # ---- the dual's rules
    row(D, 200, 300, dict(HYBRID, dual_maxviol=1, dual_bflip=0), flags=MAXVIOL),
    row(P, 200, 300, dict(HYBRID, dual_maxviol=0), flags=MAXVIOL),
    row(D, 100, 300, dict(K_SMALL, dual_bflip=1), flags=BFLIP),
    row(D, 200, 300, dict(K_MID, dual_bflip=1), flags=BFLIP),
    row(D, 1024, 1200, dict(K_MID, dual_bflip=1, dual_maxviol=1), flags=BFLIP | MAXVIOL),
    row(D, 200, 300, dict(K_MID, dual_bflip=1), flags=BFLIP, pipeline=3),
    row(D, 200, 300, dict(K_MID, dual_bflip=1), flags=BFLIP, refactor_period=50),
    row(P, 200, 300, dict(HYBRID, dual_bflip=0), flags=BFLIP),
    # ---- partial pricing (primal; a dual engine ignores it)
    row(P, 100, 300, dict(THREE, pp_P=2, pp_S=150), partial_segments=2),
    row(P, 200, 300, dict(THREE, pp_P=2, pp_S=150), partial_segments=2),
    row(P, 2000, 300, dict(THREE, pp_P=2, pp_S=150), partial_segments=2),
    row(P, 200, 300, dict(THREE, pp_P=300, pp_S=1), partial_segments=1000),
    row(P, 200, 301, dict(THREE, pp_P=101, pp_S=3), partial_segments=150),  # ceil(301 / 150) = 3 positions: 101 segments
    row(P, 200, 1, dict(HYBRID, pp_P=0), partial_segments=2),
    row(P, 200, 300, dict(THREE, pp_P=2), partial_segments=2, pipeline=3),
    row(D, 200, 300, dict(HYBRID, pp_P=0), partial_segments=2),
    # ---- a maintenance period, btran_mode 1, profiling: the explicit-inverse engine where k_small is the default
    row(P, 100, 300, dict(THREE, refactor_period=50, drift_every=0), refactor_period=50),
    row(P, 200, 300, dict(HYBRID, refactor_period=50, drift_every=0), refactor_period=50),
    row(P, 200, 300, dict(HYBRID, refactor_period=200, drift_every=64), refactor_period=200),
    row(P, 2000, 300, dict(CERT_P, refactor_period=400, drift_every=100), refactor_period=400),
    row(P, 2000, 5000, dict(CERT_P, refactor_period=0, drift_every=222)),  # the default period there: 890
    row(P, 100, 300, dict(K_SMALL, refactor_period=0), refactor_period=-1),
    row(P, 100, 300, THREE, btran_mode=1),
    row(P, 200, 300, THREE, btran_mode=1),
    row(P, 2000, 300, THREE, btran_mode=1),
    row(D, 100, 300, THREE, btran_mode=1),
    row(D, 200, 300, THREE, btran_mode=1),
    row(D, 2000, 300, dict(TWO_D, cert_large=0), btran_mode=1),
    row(P, 200, 300, K_MID, btran_mode=1, pipeline=3),
    row(P, 100, 300, THREE, profile=1),
    row(P, 200, 300, HYBRID, profile=1),
    row(D, 100, 300, THREE, profile=1),
    row(P, 100, 300, K_SMALL, profile=1, pipeline=3),
    # ---- the twelve environment variables
    row(P, 200, 300, K_MID, env={"ELLP_MID_AUTO_MAX": "200"}),
    row(D, 200, 300, K_MID, env={"ELLP_MID_AUTO_MAX": "200"}),
    row(P, 201, 300, HYBRID, env={"ELLP_MID_AUTO_MAX": "200"}),
    row(P, 200, 300, THREE, env={"ELLP_MID_AUTO_MAX": "200"}, pipeline=1),
    row(P, 100, 300, K_SMALL, env={"ELLP_MID_AUTO_MAX": ""}),
    row(P, 100, 300, dict(K_SMALL, ill_tol=0.5), env={"ELLP_ILL_TOL": "0.5"}),
    row(P, 2000, 300, dict(CERT_P, ill_tol=0.5), env={"ELLP_ILL_TOL": "0.5"}),
    row(P, 100, 300, dict(K_SMALL, ill_tol=0.0), env={"ELLP_ILL_TOL": ""}),
    row(D, 400, 500, dict(TWO_D, ill_tol=0.0, dual_fold=1), env={"ELLP_ILL_TOL": "0"}, flags=NOCERT),
    row(D, 2000, 300, dict(CERT_D, ill_tol=0.25, dual_fold=0), env={"ELLP_ILL_TOL": "0.25"}),
    row(P, 200, 300, dict(HYBRID, drift_every=7), env={"ELLP_DRIFT_EVERY": "7"}),
    row(P, 2000, 5000, dict(CERT_P, drift_every=222), env={"ELLP_DRIFT_EVERY": ""}),
    row(P, 200, 300, dict(HYBRID, drift_tol=1e-6), env={"ELLP_DRIFT_TOL": "1e-6"}),
    row(P, 200, 300, dict(HYBRID, drift_tol=1e-10), env={"ELLP_DRIFT_TOL": ""}),
    row(P, 200, 300, dict(HYBRID, unit_table=0), env={"ELLP_NO_UNIT_COLUMNS": "1"}),
    row(D, 200, 300, dict(HYBRID, unit_table=0), env={"ELLP_NO_UNIT_COLUMNS": ""}),
    row(P, 200, 300, dict(THREE, se=1, unit_table=1), env={"ELLP_NO_UNIT_COLUMNS": "1"}, flags=SE),
    row(P, 100, 300, dict(K_SMALL, stamps=1), env={"ELLP_SMALL_STAMPS": "1"}),
    row(P, 200, 300, dict(HYBRID, stamps=0), env={"ELLP_SMALL_STAMPS": "1"}),
    row(P, 200, 300, dict(K_MID, stamps=1), env={"ELLP_SMALL_STAMPS": "1"}, pipeline=3),
    row(P, 100, 300, dict(K_SMALL, small_nt=256), env={"ELLP_SMALL_NT": "256"}),
    row(P, 100, 300, dict(K_SMALL, small_nt=128), env={"ELLP_SMALL_NT": "64"}),  # fewer threads than rows: not taken
    row(P, 60, 300, dict(K_SMALL, small_nt=128), env={"ELLP_SMALL_NT": "128"}),
    row(P, 60, 300, dict(K_SMALL, small_nt=64), env={"ELLP_SMALL_NT": "96"}),
    row(P, 200, 300, THREE, env={"ELLP_NO_HYBRID": "1"}),
    row(D, 200, 300, THREE, env={"ELLP_NO_HYBRID": "1"}),
    row(P, 2000, 300, dict(TWO_P, guard_abs=0.0), env={"ELLP_NO_HYBRID": "1"}),
    row(D, 2000, 300, dict(TWO_D, cert_large=0), env={"ELLP_NO_HYBRID": ""}),
    row(P, 200, 300, dict(HYBRID, guard_abs=1e-5), env={"ELLP_GUARD_ABS": "1e-5"}),
    row(P, 2000, 300, dict(CERT_P, guard_abs=1e-5), env={"ELLP_GUARD_ABS": "1e-5"}),
    row(P, 200, 300, dict(HYBRID, guard_abs=1e-7), env={"ELLP_GUARD_ABS": ""}),
    row(P, 100, 300, dict(K_SMALL, guard_abs=0.0), env={"ELLP_GUARD_ABS": "1e-5"}),
    row(P, 200, 300, dict(HYBRID, exact_K=3), env={"ELLP_EXACT_K": "3"}),
    row(D, 2000, 300, dict(CERT_D, exact_K=3), env={"ELLP_EXACT_K": "3"}),
    row(P, 200, 300, dict(HYBRID, exact_K=8), env={"ELLP_EXACT_K": "0"}),
    row(P, 100, 300, dict(K_SMALL, exact_K=8), env={"ELLP_EXACT_K": "3"}),
    row(D, 2000, 300, dict(CERT_D, dual_fold=0), env={"ELLP_DUAL_FOLD_OFF": "1"}),
    row(D, 2000, 300, dict(CERT_D, dual_fold=1)),
    row(P, 3500, 300, dict(THREE, se=1, se_vpart=0, upd2_rows=8), env={"ELLP_SE_BTRAN": "1"}, flags=SE),
    row(P, 200, 300, dict(THREE, se=1, se_vpart=0, upd2_rows=1), env={"ELLP_SE_BTRAN": ""}, flags=SE),
]


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)


def plan(kind, m, nN, opts=None, env=None, avail=E.PLAN_AVAIL_ALL, monkeypatch=None):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return E.engine_plan(kind, m, nN, E.default_opts(**(opts or {})), avail)


def case_id(c):
    kind, m, nN, opts, env, _ = c
    return "-".join(["PD"[kind], str(m), str(nN)] + [f"{k}={v}" for k, v in opts.items()] + [f"{k[5:]}={v}" for k, v in env.items()])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_documented_modes(case, monkeypatch):
    kind, m, nN, opts, env, want = case
    s, got, msg = plan(kind, m, nN, opts, env, monkeypatch=monkeypatch)
    assert s == E.OPTIMAL, msg
    assert {k: got[k] for k in want} == {k: float(v) for k, v in want.items()}


def test_the_table_crosses_every_threshold():
    """both sides of every size at which the moved code takes another path, and every option and variable"""
    ms = {c[1] for c in CASES}
    for lo in (64, 128, 255, 383, 512, 1024, 2047, 2304, 3071, 3119, 4096):
        assert {lo, lo + 1} <= ms, lo
    assert 8192 in ms
    nNs = {c[2] for c in CASES}
    assert {0, 1, 4096, 4097, 19531, 19532, 262144, 262145} <= nNs
    assert {c[3].get("pipeline", 0) for c in CASES} == {0, 1, 2, 3}
    assert {k for c in CASES for k in c[3]} >= {"pipeline", "flags", "partial_segments", "refactor_period", "btran_mode", "profile"}
    assert {k for c in CASES for k in c[4]} == set(ENV_VARS)
    assert {c[0] for c in CASES} == {P, D}


def random_inputs(count, seed):
    rng = np.random.default_rng(seed)
    sizes = [1, 3, 64, 65, 128, 129, 255, 256, 383, 384, 512, 513, 1024, 1025, 2048, 3071, 3072, 4096, 4097, 8192]
    cols = [0, 1, 2, 63, 300, 4096, 4097, 20000, 70000, 262145]
    for _ in range(count):
        m = int(rng.choice(sizes)) if rng.random() < 0.6 else int(rng.integers(1, 8193))
        nN = int(rng.choice(cols)) if rng.random() < 0.6 else int(rng.integers(0, 30000))
        flags = int(rng.integers(0, 32))
        opts = dict(pipeline=int(rng.integers(0, 4)), flags=flags, partial_segments=int(rng.choice([0, 1, 2, 7, 100000])),
                    refactor_period=int(rng.choice([0, 0, 50, 400])), btran_mode=int(rng.choice([0, 0, 1])),
                    profile=int(rng.choice([0, 0, 1])))
        yield int(rng.integers(0, 2)), m, nN, opts, int(rng.integers(0, 4))


def test_invariants():
    planned = 0
    for kind, m, nN, opts, avail in random_inputs(4000, 20260419):
        s, p, msg = E.engine_plan(kind, m, nN, E.default_opts(**opts), avail)
        if s != E.OPTIMAL:
            assert s in (E.ERR_ARG, E.ERR_DEVICE) and msg
            continue
        planned += 1
        ctx = (kind, m, nN, opts, avail, p)
        assert p["small"] + p["hybrid"] + p["cert_large"] + p["exact_large_always"] <= 1, ctx
        assert not p["mid"] or p["small"], ctx
        if p["lagged"]:
            assert kind == P and not (p["small"] or p["hybrid"] or p["se"]), ctx
        assert not p["dual_fold"] or p["dual_fused"], ctx
        if p["dual_fused"]:
            assert kind == D and p["ld"] <= 4096, ctx
        assert not (p["price_wave"] and p["price_nt"]), ctx
        assert not p["se"] or p["pp_P"] <= 1, ctx
        assert p["upd2_blocks"] * p["upd2_rows"] >= m and p["upd_blocks"] * p["upd_rows"] >= m, ctx
        assert p["nblocks"] * p["cpb"] >= max(nN, 1), ctx
        assert p["btran_tiles"] * p["btran_rows"] >= m and p["ld"] >= m and p["ld"] % 16 == 0, ctx
        assert p["seg"] == 2 * p["nbs"] * (1 + p["cpb"]), ctx
    assert planned > 2000


def test_missing_resources_downgrade_or_refuse():
    ALL, NO_SMALL, NO_MID, NONE = 3, E.PLAN_AVAIL_MID, E.PLAN_AVAIL_SMALL, 0
    # k_small's LDS attribute refused: the explicit-inverse engine (no hybrid at these sizes: k_mid starts at 129 rows)
    for avail, want in ((ALL, K_SMALL), (NO_MID, K_SMALL), (NO_SMALL, THREE), (NONE, THREE)):
        s, p, _ = E.engine_plan(P, 100, 300, None, avail)
        assert s == E.OPTIMAL and {k: p[k] for k in want} == {k: float(v) for k, v in want.items()}, avail
    s, p, _ = E.engine_plan(P, 100, 300, E.default_opts(pipeline=2), NO_SMALL)
    assert s == E.OPTIMAL and p["lagged"] == 1  # the mask takes nothing the plan did not ask for
    # k_mid's resources refused: the hybrid becomes the plain explicit-inverse engine, two launches from 384 rows
    for kind, m, want in ((P, 200, THREE), (D, 200, THREE), (P, 500, TWO_P), (D, 500, TWO_D)):
        for avail in (NO_MID, NONE):
            s, p, _ = E.engine_plan(kind, m, 600, None, avail)
            assert s == E.OPTIMAL and {k: p[k] for k in want} == {k: float(v) for k, v in want.items()}, (kind, m, avail)
        s, p, _ = E.engine_plan(kind, m, 600, None, NO_SMALL)
        assert s == E.OPTIMAL and p["hybrid"] == 1
    # ... pipeline 3 and bound flipping insist on k_mid
    for kind, opts in ((P, dict(pipeline=3)), (D, dict(pipeline=3)), (D, dict(flags=BFLIP)), (D, dict(flags=BFLIP, pipeline=3))):
        s, p, msg = E.engine_plan(kind, 200, 300, E.default_opts(**opts), NO_MID)
        assert s == E.ERR_DEVICE and p is None
        assert "pipeline 3: no device memory for the factors of the persistent-workgroup loop" in msg
        assert E.engine_plan(kind, 200, 300, E.default_opts(**opts), NO_SMALL)[0] == E.OPTIMAL
    # bound flipping without k_small: no kernel with the long-step ratio test is left
    s, _, msg = E.engine_plan(D, 100, 300, E.default_opts(flags=BFLIP), NO_SMALL)
    assert s == E.ERR_ARG and "ELLP_FLAG_DUAL_BOUND_FLIPPING: the LU-per-iteration kernels take up to 1,024 rows" in msg
    # above 1,024 rows nothing is asked of either
    for avail in (ALL, NO_SMALL, NO_MID, NONE):
        s, p, _ = E.engine_plan(P, 2000, 300, None, avail)
        assert s == E.OPTIMAL and p["cert_large"] == 1 and p["lagged"] == 1


TILE = "m = 8193 exceeds this build's pricing tile (m <= 8192)"
BFLIP_PIPE = ("ELLP_FLAG_DUAL_BOUND_FLIPPING runs on the LU-per-iteration kernels (pipeline 0 or 3, up to 1,024 rows), "
              "not on the explicit-inverse pipelines 1 / 2")
SE_TEXT = ("ELLP_FLAG_PRIMAL_STEEPEST_EDGE runs on the three-launch pipeline (pipeline 0 or 1) with full "
           "pricing and the incremental BTRAN: not with partial_segments > 1, pipeline 2 / 3 or btran_mode 1")
BFLIP_ROWS = "ELLP_FLAG_DUAL_BOUND_FLIPPING: the LU-per-iteration kernels take up to 1,024 rows (this LP: 1025)"

REFUSALS = [
    (P, 8193, 10, {}, TILE),
    (D, 8193, 10, {}, TILE),
    (D, 200, 300, dict(flags=BFLIP, pipeline=1), BFLIP_PIPE),
    (D, 200, 300, dict(flags=BFLIP, pipeline=2), BFLIP_PIPE),
    (P, 200, 300, dict(flags=SE, partial_segments=2), SE_TEXT),
    (P, 200, 300, dict(flags=SE, pipeline=2), SE_TEXT),
    (P, 200, 300, dict(flags=SE, pipeline=3), SE_TEXT),
    (P, 200, 300, dict(flags=SE, btran_mode=1), SE_TEXT),
    (P, 200, 0, dict(flags=SE, pipeline=2), SE_TEXT),
    (D, 1025, 1200, dict(flags=BFLIP), BFLIP_ROWS),
    (D, 1025, 1200, dict(flags=BFLIP, pipeline=3), BFLIP_ROWS),
    # two faults: the earlier refusal answers
    (D, 8193, 10, dict(flags=BFLIP, pipeline=1), TILE),
    (P, 8193, 10, dict(flags=SE, pipeline=2), TILE),
    (D, 1025, 1200, dict(flags=BFLIP, pipeline=2), BFLIP_PIPE),
]


@pytest.mark.parametrize("kind,m,nN,opts,text", REFUSALS)
def test_refusals(kind, m, nN, opts, text):
    s, p, msg = E.engine_plan(kind, m, nN, E.default_opts(**opts))
    assert s == E.ERR_ARG and p is None and text in msg


def test_bad_arguments():
    for args in ((2, 10, 10), (P, 0, 10), (P, 10, -1)):
        s, p, msg = E.engine_plan(*args)
        assert s == E.ERR_ARG and msg
    import ctypes as C
    out = np.zeros(10)
    err = C.create_string_buffer(64)
    assert E.lib().ellp_engine_plan(P, 10, 10, None, 3, E._p(out), out.size, err, 64) == E.ERR_ARG
    assert E.lib().ellp_engine_plan(P, 10, 10, None, 3, None, 47, err, 64) == E.ERR_ARG


def test_creation_refuses_before_any_device_work():
    """ellp_engine_create answers a refused combination with the plan's status and text on any machine, and the dual's
    starting point is judged before the options: the order of creation's refusals"""
    for kind, opts, text in ((D, dict(flags=BFLIP, pipeline=1), BFLIP_PIPE), (P, dict(flags=SE, pipeline=2), SE_TEXT)):
        fp = unit_basis_problem(kind, 5, 7)
        with pytest.raises(E.EllpHipError) as ei:
            E.Engine(kind, fp, E.default_opts(**opts))
        assert ei.value.status == E.ERR_ARG and ei.value.msg == E.engine_plan(kind, 5, 7, E.default_opts(**opts))[2] and text in ei.value.msg
    fp = unit_basis_problem(D, 5, 7)
    fp.d[:] = -1.0
    with pytest.raises(E.EllpHipError) as ei:
        E.Engine(D, fp, E.default_opts(flags=BFLIP, pipeline=1))
    assert ei.value.status == E.ERR_PANIC and "dual infeasible" in ei.value.msg
