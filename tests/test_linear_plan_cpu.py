"""linear_plan is host arithmetic: the plan cases of test_gpu_linear_dma.py
hold without a device."""
import itertools

import pytest

from ddp_tricks_amd.ops import load_extension

from test_gpu_linear_dma import (BENCH_SHAPES, DGRAD, FWD, GEMM, K_EDGES,
                                 MN_EDGES, ROUTED, WGRAD)

ext = load_extension(required=True)


def test_benchmarked_shapes_follow_the_routing_table():
    for M, N, K in BENCH_SHAPES:
        for op in (FWD, DGRAD, WGRAD):
            assert ext.linear_plan(op, M, N, K) == ROUTED[op]
            assert ext.linear_plan(op, M, N, K, -1) == ROUTED[op]
            assert ext.linear_plan(op, M, N, K, 0) == "legacy"
            assert ext.linear_plan(op, M, N, K, 1) == "dma"


def test_forced_dma_fits_every_edge_shape():
    for gm, gn, gk in itertools.product(MN_EDGES, MN_EDGES, K_EDGES):
        assert ext.linear_plan(GEMM, gm, gn, gk, 1) == "dma"
        want = "dma" if gn > 16 else "legacy"
        for op in (FWD, DGRAD, WGRAD):
            assert ext.linear_plan(op, gm, gn, gk, 1) == want


@pytest.mark.parametrize("mnk", [(100, 70, 130), (128, 128, 68),
                                 (128, 132, 64), (128, 128, 4)])
def test_forced_dma_on_a_misfit_reports_legacy(mnk):
    for op in (FWD, DGRAD, WGRAD, GEMM):
        for impl in (-1, 0, 1):
            assert ext.linear_plan(op, *mnk, impl) == "legacy"


def test_small_head_is_not_planned():
    for op in (FWD, DGRAD, WGRAD):
        for N in (8, 10, 16):
            for impl in (-1, 0, 1):
                assert ext.linear_plan(op, 1024, N, 512, impl) == "legacy"
        assert ext.linear_plan(op, 1024, 24, 512, 1) == "dma"


def test_bad_arguments_raise():
    for bad in (-2, 2, 7):
        with pytest.raises(RuntimeError):
            ext.linear_plan(FWD, 128, 128, 64, bad)
    for op in (-1, 4):
        with pytest.raises(RuntimeError):
            ext.linear_plan(op, 128, 128, 64, -1)
