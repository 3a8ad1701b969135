"""Host plan queries of the convolution dispatchers (no GPU): pinned at the dispatch thresholds, the Python mirrors in ops agree with
them, and the cases of tests/test_exact_conv_kernels.py reach every branch and every plan a bench step launches."""
import pytest

from conv_geometries import bench_geometries, bf16_plan, halo_shape, wgrad_plan


@pytest.fixture
def lib():
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    yield lib
    lib.ssd_tune_set_conv_bf16(-1, -1)
    lib.ssd_tune_set_conv_bf16_k64(1)
    lib.ssd_tune_set_wgrad(-1, -1, -1)
    lib.ssd_tune_set_wgrad_patch(-1)
    lib.ssd_tune_set_halo(-1)


def test_bench_geometries_are_the_model_s():
    geos = bench_geometries(300, 32, (21,))
    assert (32, 300, 300, 64, 64, 3, 1, 1, 1) in geos and (32, 19, 19, 512, 1024, 3, 1, 4, 4) in geos
    assert (32, 38, 38, 512, 100, 3, 1, 1, 1) in geos and (32, 19, 19, 1024, 150, 3, 1, 1, 1) in geos
    assert (32, 3, 3, 128, 256, 3, 1, 0, 1) in geos
    geos = bench_geometries(512, 16, (21, 81))
    assert (16, 512, 512, 64, 64, 3, 1, 1, 1) in geos and (16, 64, 64, 512, 340, 3, 1, 1, 1) in geos


def test_bf16_tensor_conv_plan_at_its_thresholds(lib):
    # flat space while 256 + 2 (W + 1) + 2 rows fit: 6 pieces to W = 62, 7 to W = 94; then 16x16 patches, 8x32 from H, W >= 128
    assert bf16_plan(16, 62, 62, 64, 128) == (2, 128, 6, 0)
    assert bf16_plan(16, 63, 63, 64, 128) == (2, 128, 7, 0)
    assert bf16_plan(16, 94, 94, 64, 128) == (2, 128, 7, 0)
    assert bf16_plan(16, 95, 95, 64, 128) == (1, 128, 6, 0)
    assert bf16_plan(2, 127, 128, 64, 128) == (1, 128, 6, 0) and bf16_plan(2, 128, 127, 64, 128) == (1, 128, 6, 0)
    assert bf16_plan(2, 128, 128, 64, 128) == (0, 128, 6, 0)
    # 64 output channels: the flat form has 6-piece buffers only; K = 64 with <= 64 outputs on 8x32 patches is the persistent kernel
    assert bf16_plan(8, 62, 62, 64, 64) == (2, 64, 6, 0) and bf16_plan(8, 63, 63, 64, 64) == (1, 64, 6, 0)
    assert bf16_plan(2, 128, 128, 64, 64) == (0, 64, 6, 1) and bf16_plan(2, 128, 128, 128, 64) == (0, 64, 10, 0)
    lib.ssd_tune_set_conv_bf16_k64(0)
    assert bf16_plan(2, 128, 128, 64, 64) == (0, 64, 10, 0)
    lib.ssd_tune_set_conv_bf16_k64(1)
    # the block-count switch: <= 128 blocks of 128-channel flat tiles take 64-channel tiles
    assert bf16_plan(81, 19, 19, 512, 128) == (2, 64, 6, 0) and bf16_plan(82, 19, 19, 512, 128) == (2, 128, 6, 0)
    # forced
    lib.ssd_tune_set_conv_bf16(2, 128)
    assert bf16_plan(1, 200, 200, 64, 128) == (1, 128, 6, 0)          # a flat space that does not fit falls back to patches
    lib.ssd_tune_set_conv_bf16(0, 64)
    assert bf16_plan(1, 8, 32, 64, 64) == (0, 64, 6, 1)


def test_weight_gradient_plan_at_its_thresholds(lib):
    # bf16: the patch kernel for 3x3 (padding = dilation 1 or 4) and 1x1 stride-1 layers, its form, the f32 kernels elsewhere
    assert wgrad_plan((32, 300, 300, 64, 64, 3, 1, 1, 1), True)[:5] == (2, 64, 1, -1, 0)
    assert wgrad_plan((32, 19, 19, 512, 1024, 3, 1, 4, 4), True)[:5] == (2, 64, 1, -1, 1)
    assert wgrad_plan((32, 19, 19, 1024, 1024, 1, 1, 0, 1), True)[:5] == (2, 64, 1, -1, 2)
    assert wgrad_plan((32, 19, 19, 256, 512, 3, 2, 1, 1), True)[0] == 0
    # f32: the nine-tap kernel with the least-padding patch shape (ties: 2x19, then 1x38) up to 12 % waste
    assert wgrad_plan((32, 38, 38, 512, 512, 3, 1, 1, 1), False)[:4] == (1, 64, 1, 2)     # 1x38 and 2x19 both exact: 2x19
    assert wgrad_plan((32, 75, 75, 256, 256, 3, 1, 1, 1), False)[:4] == (1, 64, 1, 1)     # 1x38: 1.3 % against 2.7 % and 8.1 %
    assert wgrad_plan((32, 64, 64, 256, 256, 3, 1, 1, 1), False)[:4] == (1, 64, 1, 0)     # 4x8 tiles 64 x 64 exactly
    assert wgrad_plan((32, 5, 5, 128, 256, 3, 1, 1, 1), False)[0] == 0          # 4x8: 60 % padding -> one tap per block
    assert wgrad_plan((32, 10, 10, 512, 256, 3, 2, 1, 1), False)[:2] == (0, 128)
    assert wgrad_plan((32, 10, 10, 512, 150, 3, 2, 1, 1), False)[:2] == (0, 64)  # 150 rows: 64-row tiles
    # splits: at least 4 patches per block (npatch / 4), at most 1024; the tap-wise reduction for < 512 blocks and >= 32 splits
    pl = wgrad_plan((2, 19, 19, 64, 64, 3, 1, 1, 1), True)
    assert pl[5] <= 30 // 4 and pl[6] >= 4 and pl[7] == 0
    lib.ssd_tune_set_wgrad(-1, -1, 40)
    assert wgrad_plan((8, 136, 128, 64, 64, 3, 1, 1, 1), True)[5:7] == (871, 5)      # 1024 cap: 4352 patches / 1024 -> 5 per split
    assert wgrad_plan((8, 128, 128, 64, 64, 3, 1, 1, 1), True)[5:7] == (1024, 4)     # 4096 patches: both caps at 1024
    lib.ssd_tune_set_wgrad(-1, -1, -1)
    assert wgrad_plan((32, 300, 300, 64, 64, 3, 1, 1, 1), True)[7] == 1
    assert wgrad_plan((32, 38, 38, 512, 512, 3, 1, 1, 1), True)[7] == 0


def test_halo_acceptance_at_its_thresholds(lib):
    assert [halo_shape((1, 30, 64, 64, 64, 3, 1, 1, 1), 0, p) for p in (1, 3)] == [2, 2]
    assert [halo_shape((1, 29, 64, 64, 64, 3, 1, 1, 1), 0, p) for p in (1, 3)] == [0, 0]
    assert [halo_shape((1, 30, 63, 64, 64, 3, 1, 1, 1), 0, p) for p in (1, 3)] == [2, 0]
    assert [halo_shape((1, 30, 29, 64, 64, 3, 1, 1, 1), 0, p) for p in (1, 3)] == [0, 0]
    assert halo_shape((1, 64, 64, 64, 64, 3, 2, 1, 1), 1, 1) == 0 and halo_shape((1, 64, 64, 64, 64, 3, 1, 4, 4), 0, 1) == 0
    lib.ssd_tune_set_halo(1)
    assert halo_shape((1, 8, 8, 64, 64, 3, 1, 1, 1), 0, 3) == 1
    lib.ssd_tune_set_halo(0)
    assert halo_shape((1, 300, 300, 64, 64, 3, 1, 1, 1), 0, 3) == 0


GRID = [(n, h, w, ci, co, k, s, p, d) for n in (1, 32) for h, w in ((3, 3), (19, 19), (29, 64), (30, 63), (30, 64), (38, 38), (75, 75), (300, 300))
        for ci, co in ((64, 64), (96, 150), (512, 512), (1024, 100)) for k, s, p, d in ((3, 1, 1, 1), (3, 2, 1, 1), (1, 1, 0, 1), (3, 1, 4, 4))
        if h + 2 * p - d * (k - 1) > 0]


def test_ops_mirrors_agree_with_the_library():
    from objectdetection_ssd_amd import ops
    for geo in GRID:
        g = ops.make_geom(*geo)
        for direction in (0, 1):
            for bf16, x3, planes in ((True, False, 1), (False, True, 3)):
                halo = halo_shape(geo, direction, planes) > 0 and (direction == 1 or g.Ci % 32 == 0)
                assert (ops.igemm_tile(g, direction, bf16, x3) == "conv3x3_halo_kernel") == halo, (geo, direction, planes)
        for bf16 in (False, True):
            pl = wgrad_plan(geo, bf16)
            name = ops.wgrad_tile(g, bf16)
            want = "wgrad3x3_bf16_kernel" if pl[0] == 2 else ("wgrad3x3_kernel" if pl[0] == 1 else f"wgrad_kernel<{pl[1]}")
            assert name == want, (geo, bf16, name, want)


def _verified_bf16_plans(lib):
    """every plan the bf16-tensor convolution cases of tests/test_exact_conv_kernels.py run (same forced settings)"""
    import test_exact_conv_kernels as T
    seen = set()
    runs = [((n, h, w, ci, co), T.BF16_FORCED, (1, 0), co) for (n, h, w, ci, co), _ in T.BF16T_CASES]
    runs += [((2, 19, 19, 256, co), [(-1, -1), (2, 64), (2, 128), (1, 128)], (1,), n_out) for co, n_out in T.HEAD_CASES]
    runs += [((n, h, w, 64, 64), [(0, 64)], (1,), 64) for n, h, w in T.K64_CASES]
    runs += [((bs, h, w, ci, co), [(-1, -1)], (1,), (co + 3) // 4 * 4)
             for v, batch in T.BENCH_RUNS for bs, h, w, ci, co, k, s, p, d in bench_geometries(v, batch, (21, 81))
             if (k, s, p, d) == (3, 1, 1, 1) and ci % 64 == 0]
    try:
        for (n, h, w, ci, co), forced, k64s, n_out in runs:
            for on in k64s:
                lib.ssd_tune_set_conv_bf16_k64(on)
                for mode, bn in forced:
                    lib.ssd_tune_set_conv_bf16(mode, bn)
                    seen.add(bf16_plan(n, h, w, ci, n_out))                        # forward
                    seen.add(bf16_plan(n, h, w, (co + 63) // 64 * 64, ci))         # flipped-tap data gradient
    finally:
        lib.ssd_tune_set_conv_bf16(-1, -1)
        lib.ssd_tune_set_conv_bf16_k64(1)
    return seen


def test_exact_cases_cover_every_bf16_conv_plan_and_every_bench_plan(lib):
    import test_exact_conv_kernels as T
    seen = _verified_bf16_plans(lib)
    reachable = {(0, 64, 10, 0), (1, 64, 6, 0), (2, 64, 6, 0), (0, 128, 6, 0), (1, 128, 6, 0), (2, 128, 6, 0), (2, 128, 7, 0), (0, 64, 6, 1)}
    assert reachable <= seen, reachable - seen
    bench = set()
    for v, batch in T.BENCH_RUNS:
        for n, h, w, ci, co, k, s, p, d in bench_geometries(v, batch, (21, 81)):
            if (k, s, p, d) == (3, 1, 1, 1) and ci % 64 == 0:
                bench.add(bf16_plan(n, h, w, ci, (co + 3) // 4 * 4))
                bench.add(bf16_plan(n, h, w, (co + 63) // 64 * 64, ci))
    assert bench <= seen, bench - seen


def test_exact_cases_cover_every_weight_gradient_branch_the_bench_takes():
    import test_exact_conv_kernels as T
    key = lambda pl: pl[:5] + pl[7:]                   # noqa: E731  (everything but the split counts)
    cases = T.EDGE_CASES + T.WGRAD_BF16_CASES + [g for v, bs in T.BENCH_RUNS for g in bench_geometries(v, bs, (21, 81))]
    seen = {key(wgrad_plan(g, b)) for g in cases for b in (False, True)}
    for v, batch in T.BENCH_RUNS:
        for geo in bench_geometries(v, batch, (21, 81)):
            for b in (False, True):
                assert key(wgrad_plan(geo, b)) in seen
    assert {0, 1} <= {k[-1] for k in seen}                     # both reduction forms
    assert {0, 1, 2} <= {k[4] for k in seen if k[0] == 2}      # all three bf16 patch forms
