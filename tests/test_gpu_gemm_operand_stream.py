"""The operand stream of the 256x256 LDS-DMA GEMM (gemm_bf16_v4): every piece is fetched from a 64-bit scalar base (the
operand pointer plus the K-slice's and the k-tile's offset) plus a 32-bit per-lane byte offset.  Integer-valued bf16
operands make every product and fp32 sum exact, so an addressing error shows as a wrong value against the fp64 product
(torch.equal), never as a tolerance miss."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from VisionTransformer import _ops  # noqa: E402

DEV = "cuda"
LAYOUTS = [(True, True), (True, False), (False, False)]          # the bf16 layouts the library provides
ALL_LAYOUTS = LAYOUTS + [(False, True)]                           # (A row-strided, B k-contiguous): refused for bf16


def _ints(shape, gen, lo=-4, hi=5, dtype=torch.bfloat16):
    return torch.randint(lo, hi, shape, generator=gen).to(dtype).to(DEV)


def _ref(A, B, akc, bkc):
    """C[i][j] = sum_r A(i,r) B(j,r) in float64 from the stored layouts."""
    Ai = A.double() if akc else A.double().t()
    Bj = B.double() if bkc else B.double().t()
    return Ai @ Bj.t()


@pytest.mark.parametrize("akc,bkc", ALL_LAYOUTS)
@pytest.mark.parametrize("n", range(1, 13))
def test_k_sweep(libopt, akc, bkc, n):
    """M = N = 256, K = 64 n: n = 1..8 are every prologue / tail length of the 8-slot ring, 9..12 reach the steady
    loop.  fp32 and bf16 outputs (the one-item-per-workgroup and the persistent wide-epilogue kernels)."""
    libopt("gemm_impl", 4)
    M = N = 256
    K = 64 * n
    g = torch.Generator().manual_seed(100 * n + 2 * akc + bkc)
    A = _ints((M, K) if akc else (K, M), g)
    B = _ints((N, K) if bkc else (K, N), g)
    C = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    if not akc and bkc:
        with pytest.raises(RuntimeError):
            _ops.gemm(A, B, C, M, N, K, A.stride(0), B.stride(0), N, a_kcontig=akc, b_kcontig=bkc)
        return
    ref = _ref(A, B, akc, bkc)
    _ops.gemm(A, B, C, M, N, K, A.stride(0), B.stride(0), N, a_kcontig=akc, b_kcontig=bkc)
    assert torch.equal(C.double(), ref), (C.double() - ref).abs().max()
    Cb = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    _ops.gemm(A, B, Cb, M, N, K, A.stride(0), B.stride(0), N, a_kcontig=akc, b_kcontig=bkc)
    assert torch.equal(Cb, ref.float().bfloat16())


@pytest.mark.parametrize("akc,bkc", LAYOUTS)
@pytest.mark.parametrize("n,split", [(11, 3), (7, 4)])
def test_k_sweep_split_k_uneven(libopt, akc, bkc, n, split):
    """Split-K with an uneven last slice (11 k-tiles as 4 + 4 + 3, 7 as 2 + 2 + 2 + 1): a slice's first k-tile is not
    the operand's, so its offset goes through the scalar base."""
    libopt("gemm_impl", 4)
    M = N = 256
    K = 64 * n
    g = torch.Generator().manual_seed(1000 * split + n + 2 * akc + bkc)
    A = _ints((M, K) if akc else (K, M), g)
    B = _ints((N, K) if bkc else (K, N), g)
    C = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(split * M * N, dtype=torch.float32, device=DEV)
    _ops.gemm(A, B, C, M, N, K, A.stride(0), B.stride(0), N, a_kcontig=akc, b_kcontig=bkc, split_k=split,
              workspace=ws)
    ref = _ref(A, B, akc, bkc)
    assert torch.equal(C.double(), ref), (C.double() - ref).abs().max()


@pytest.mark.parametrize("bkc", [True, False])
@pytest.mark.parametrize("M,N", [(1024, 768), (4608, 3840)])
def test_persistent_items(libopt, bkc, M, N):
    """A persistent kind (bf16 output, plain epilogue), K = 192: a workgroup computes the next item's lane offsets and
    scalar bases while the previous tile's epilogue runs.  1024 x 768 is 12 items (one per workgroup on a chip with
    more CUs than that); 4608 x 3840 is 270 items, more than the 256 CUs, so the grid is smaller than the item count
    and some workgroups take a second item.  Bitwise equal to the one-workgroup-per-item launch and to the exact
    product."""
    libopt("gemm_impl", 4)
    K = 192
    g = torch.Generator().manual_seed(M + N + bkc)
    A = _ints((M, K), g)
    B = _ints((N, K) if bkc else (K, N), g)
    outs = []
    for persist in (1, 0):
        libopt("gemm_persist", persist)
        C = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        _ops.gemm(A, B, C, M, N, K, K, B.stride(0), N, b_kcontig=bkc)
        outs.append(C)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], _ref(A, B, True, bkc).float().bfloat16())


@pytest.mark.parametrize("akc,bkc", LAYOUTS)
def test_sub_views(libopt, akc, bkc):
    """A and B are views that start 16-B aligned deep inside a larger allocation, with leading dimensions 64 elements
    larger than the contiguous extent; everything around them is NaN.  The scalar base must be the view's pointer, and
    M = 200 / N = 136 have clamped edge rows."""
    libopt("gemm_impl", 4)
    M, N, K = 200, 136, 192
    g = torch.Generator().manual_seed(5 + 2 * akc + bkc)

    def view(rows, cols, start):
        ld = cols + 64
        buf = torch.full((start + rows * ld + 4096,), float("nan"), dtype=torch.bfloat16, device=DEV)
        v = buf[start:start + rows * ld].view(rows, ld)[:, :cols]
        v.copy_(_ints((rows, cols), g))
        assert v.data_ptr() % 16 == 0 and v.data_ptr() - buf.data_ptr() == 2 * start
        return buf, v, ld

    _, A, lda = view(*((M, K) if akc else (K, M)), start=1_000_008)
    _, B, ldb = view(*((N, K) if bkc else (K, N)), start=3_000_040)
    ref = _ref(A, B, akc, bkc)
    C = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    _ops.gemm(A, B, C, M, N, K, lda, ldb, N, a_kcontig=akc, b_kcontig=bkc)
    assert torch.equal(C.double(), ref), (C.double() - ref).abs().max()
    Cb = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    _ops.gemm(A, B, Cb, M, N, K, lda, ldb, N, a_kcontig=akc, b_kcontig=bkc)
    assert torch.equal(Cb, ref.float().bfloat16())


# One operand just under the LDS-DMA path's 2 GiB limit: [349,440 x 3072] bf16 = 2,146,959,360 B, so the lane offsets
# of its last rows have bit 30 set and the k-tile offsets of the row-strided use reach 2.1e9.
BIG_ROWS, BIG_COLS = 349_440, 3072


@pytest.fixture(scope="module")
def big_operand():
    """About 2.2 GB for the operand; with the outputs and the split-K slabs the two tests need about 3 GB of device
    memory.  Skipped when the allocation fails."""
    try:
        A = torch.randint(-4, 5, (BIG_ROWS, BIG_COLS), device=DEV, dtype=torch.bfloat16,
                          generator=torch.Generator(device=DEV).manual_seed(3))
    except torch.OutOfMemoryError:
        pytest.skip("needs about 3 GB of free device memory")
    assert A.numel() * 2 < 0x7fffffff and (BIG_ROWS - 1) * BIG_COLS * 2 >= 1 << 30
    yield A
    del A
    torch.cuda.empty_cache()


def test_offsets_bit30_k_contiguous(libopt, big_operand):
    """The big operand as k-contiguous A (M = 349,440, K = 3072) against N = 256: the last 256 output rows (lane
    offsets of 2.1e9) against the product of those rows, on the fp32 (one item per workgroup) and the bf16
    (persistent, 1365 items) kernels."""
    libopt("gemm_impl", 4)
    A = big_operand
    M, K, N = BIG_ROWS, BIG_COLS, 256
    B = _ints((N, K), torch.Generator().manual_seed(4))
    ref = A[-256:].double() @ B.double().t()
    for dtype in (torch.float32, torch.bfloat16):
        C = torch.empty(M, N, dtype=dtype, device=DEV)
        _ops.gemm(A, B, C, M, N, K, K, K, N)
        assert torch.equal(C[-256:], ref.to(dtype) if dtype == torch.float32 else ref.float().bfloat16())
        del C


@pytest.mark.parametrize("split", [1, 16])
def test_offsets_bit30_row_strided(libopt, big_operand, split):
    """The same memory as the row-strided A of a weight-gradient-shaped call (K = 349,440, M = 3072, N = 256, fp32
    output): the k-tile offset grows to the operand's size in the scalar base, and with split 16 each slice starts
    342 k-tiles further in.  B is zero except its last 1024 rows, so the output is the contribution of the last 16
    k-tiles, checked against the product of that slice."""
    libopt("gemm_impl", 4)
    A = big_operand
    K, M, N, S = BIG_ROWS, BIG_COLS, 256, 1024
    B = torch.zeros(K, N, dtype=torch.bfloat16, device=DEV)
    B[-S:] = _ints((S, N), torch.Generator().manual_seed(6))
    ref = A[-S:].double().t() @ B[-S:].double()
    C = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    _ops.gemm(A, B, C, M, N, K, M, N, N, a_kcontig=False, b_kcontig=False, split_k=split)
    assert torch.equal(C.double(), ref), (C.double() - ref).abs().max()
