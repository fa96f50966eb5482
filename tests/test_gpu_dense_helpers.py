"""The dense helpers of the training heads through the C ABI, each on its own: ``ihmr_transpose``, ``ihmr_colsum`` and
``ihmr_relu_backward`` in each of the forms its entry point chooses between (csrc/train.h, csrc/ihmr_hip.hip).  Outputs live
inside larger allocations filled with a sentinel bit pattern: what the call may not write must come back unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x4B1D5EA7               # a finite float (1.03e7): a sentinel that is read by mistake changes a sum visibly
SENT_F = np.array([SENTINEL], np.int32).view(np.float32)[0]


def _ceil(a, b):
    return -(-a // b) * b


class _Buf:
    """`count` floats on the device, `lead` sentinel floats before and GUARD after them; everything starts as the sentinel."""

    def __init__(self, count, lead=GUARD):
        self.count, self.lead = count, lead
        self.full = torch.full((lead + count + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.t = self.full[lead:lead + count].view(torch.float32)

    def put(self, host):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(host, np.float32).reshape(-1)))
        return self

    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def bits(self):
        """int32 bits of the payload; asserts both guards on the way."""
        f = self.full.cpu().numpy()
        assert (f[:self.lead] == SENTINEL).all() and (f[self.lead + self.count:] == SENTINEL).all(), "guard overwritten"
        return f[self.lead:self.lead + self.count].copy()


def _lib():
    from ihmr_amd import hip
    return hip.lib(), hip.stream_ptr()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------ ihmr_transpose
TRANSPOSE_SIZES = [(1, 1), (31, 33), (32, 32), (33, 31), (20, 1152), (512, 1152), (90, 512)]


@pytest.mark.parametrize("padded", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("rows,cols", TRANSPOSE_SIZES)
def test_transpose_is_bit_identical_and_writes_nothing_else(rows, cols, padded):
    """y[c][r] = x[r][c] bit for bit (-0.0, denormals and infinities included), once with ldx = cols, ldy = rows and once with
    both strides larger (ldy a multiple of 16 above rows, as the trainers' transposed operands; ldx odd, so the rows of x are
    not 16-byte aligned).  y starts as a sentinel: the stride gaps and 64 floats at both ends keep it."""
    L, st = _lib()
    ldx, ldy = (cols + 5, _ceil(rows + 1, 16)) if padded else (cols, rows)
    rng = np.random.RandomState(rows * 10007 + cols)
    x = rng.normal(0, 1, (rows, ldx)).astype(np.float32)
    idx = np.arange(0, x.size, 11)
    x.reshape(-1)[idx] = np.array([-0.0, 1e-45, -3e-40, np.inf, 1.17549435e-38, 3e38, -np.inf], np.float32)[np.arange(idx.size) % 7]
    xb = _Buf(rows * ldx).put(x)
    yb = _Buf(cols * ldy)
    assert L.ihmr_transpose(xb.ptr(), yb.ptr(), rows, cols, ldx, ldy, st) == 0
    torch.cuda.synchronize()
    y = yb.bits().reshape(cols, ldy)
    assert np.array_equal(y[:, :rows], _bits(x[:, :cols].T)), "transpose differs from x.t()"
    assert (y[:, rows:] == SENTINEL).all(), "a stride gap of y was written"
    assert np.array_equal(xb.bits(), _bits(x).reshape(-1)), "x was written"


def test_transpose_refuses_short_strides():
    L, st = _lib()
    rows, cols = 20, 33
    xb, yb = _Buf(rows * cols).put(np.ones(rows * cols)), _Buf(cols * rows)
    assert L.ihmr_transpose(xb.ptr(), yb.ptr(), rows, cols, cols - 1, rows, st) != 0          # ldx < cols
    assert L.ihmr_transpose(xb.ptr(), yb.ptr(), rows, cols, cols, rows - 1, st) != 0          # ldy < rows
    torch.cuda.synchronize()
    assert (yb.bits() == SENTINEL).all()
    assert L.ihmr_transpose(xb.ptr(), yb.ptr(), rows, cols, cols, rows, st) == 0
    torch.cuda.synchronize()
    assert (yb.bits() == _bits(np.ones(1))[0]).all()


# --------------------------------------------------------------------------------------------------------------- ihmr_colsum
COLSUM_ROWS = [1, 2, 3, 4, 5, 7, 20, 300, 512]
COLSUM_COLS = [1, 63, 64, 65, 90, 1024]


def _colsum(x, cols):
    """x (rows, ldx) host -> the entry's out[:cols] as float32; the gap columns of x and out beyond cols are checked here."""
    L, st = _lib()
    rows, ldx = x.shape
    xb = _Buf(rows * ldx).put(x)
    ob = _Buf(cols)
    assert L.ihmr_colsum(xb.ptr(), ob.ptr(), rows, cols, ldx, st) == 0
    torch.cuda.synchronize()
    return ob.bits().view(np.float32)                              # (bits() asserts that `out` beyond cols kept its sentinel)


@pytest.mark.parametrize("rows", COLSUM_ROWS)
def test_colsum_exact_on_integers_and_within_its_own_bound(rows):
    """out[c] = sum_r x[r][c] for every (cols, ldx) of the list, ldx = cols and cols + 6 (the six gap columns hold 3e38: read by
    mistake they would not go unnoticed).

    Integer-valued inputs with |x| <= 64: every partial sum is an integer below 2**24 (512 x 64 = 2**15), so every addition is
    exact in any order and the result must equal the integer sum bit for bit.

    N(0, 1) inputs against the float64 column sum, with the rigorous bound of the kernel's own order: each of the four waves
    adds its ceil(rows / 4) terms in sequence, two more additions join the four partial sums, every addition rounds by at most
    2**-24 of a partial sum that is at most sum_r |x[r][c]|:  |err| <= (ceil(rows / 4) + 2) x 2**-24 x sum_r |x[r][c]|."""
    for cols in COLSUM_COLS:
        for ldx in (cols, cols + 6):
            rng = np.random.RandomState(rows * 4099 + cols * 7 + ldx)
            xi = np.full((rows, ldx), 3e38, np.float32)
            xi[:, :cols] = rng.randint(-64, 65, (rows, cols))
            got = _colsum(xi, cols)
            want = xi[:, :cols].astype(np.int64).sum(0).astype(np.float32)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"integer column sums rows={rows} cols={cols} ldx={ldx}"
            xn = np.full((rows, ldx), 3e38, np.float32)
            xn[:, :cols] = rng.normal(0, 1, (rows, cols))
            got = _colsum(xn, cols).astype(np.float64)
            x64 = xn[:, :cols].astype(np.float64)
            bound = (-(-rows // 4) + 2) * 2.0 ** -24 * np.abs(x64).sum(0)
            err = np.abs(got - x64.sum(0))
            worst = int(np.argmax(err - bound))
            print(f"[parity] colsum rows={rows} cols={cols} ldx={ldx}: max|err| {err.max():.3e}, at the column closest to its bound "
                  f"{err[worst]:.3e} of {bound[worst]:.3e}")
            assert np.all(err <= bound), f"colsum rows={rows} cols={cols} ldx={ldx}: {err[worst]:.3e} > {bound[worst]:.3e}"


# -------------------------------------------------------------------------------------------------------- ihmr_relu_backward
def _relu_case(rows, cols, ld_dx, ld_y, lead_dx=GUARD, lead_y=GUARD):
    """Runs the entry on seeded data and compares with torch.where(y > 0, dx, 0) bit for bit.  y holds +0.0, -0.0, the smallest
    positive normal, positive and negative denormals, negative and large values (no NaN, see the test's docstring); dx holds
    ordinary values and -0.0.  The gap columns of dx (ld_dx > cols) and its guards must keep the sentinel; y comes back unchanged."""
    L, st = _lib()
    rng = np.random.RandomState(rows * 131 + cols + ld_dx)
    special = np.array([0.0, -0.0, 1.17549435e-38, 1e-45, 7e-41, -1e-45, -1.17549435e-38, -2.5, 3e38, -3e38, np.inf, -np.inf], np.float32)
    y = rng.normal(0, 1, (rows, cols)).astype(np.float32)
    pick = rng.rand(rows, cols) < 0.4
    y[pick] = special[rng.randint(0, len(special), int(pick.sum()))]
    y.reshape(-1)[:min(len(special), y.size)] = special[:min(len(special), y.size)]          # every special value at least once (size permitting)
    dx = rng.normal(0, 1, (rows, cols)).astype(np.float32)
    dx[rng.rand(rows, cols) < 0.2] = -0.0
    yf = np.full((rows, ld_y), SENT_F, np.float32)
    yf[:, :cols] = y
    yf[:, cols:] = np.where(np.arange(ld_y - cols) % 2 == 0, -1.0, 1.0)                      # gap columns of y: both signs
    dxf = np.full((rows, ld_dx), SENT_F, np.float32)
    dxf[:, :cols] = dx
    yb = _Buf(rows * ld_y, lead_y).put(yf)
    db = _Buf(rows * ld_dx, lead_dx).put(dxf)
    assert yb.full.data_ptr() % 16 == 0 and db.full.data_ptr() % 16 == 0
    assert L.ihmr_relu_backward(db.ptr(), yb.ptr(), rows, cols, ld_dx, ld_y, st) == 0
    torch.cuda.synchronize()
    want = torch.where(torch.from_numpy(y) > 0, torch.from_numpy(dx), torch.zeros(())).numpy()
    got = db.bits().reshape(rows, ld_dx)
    assert np.array_equal(got[:, :cols], _bits(want)), f"relu backward {rows}x{cols} ld {ld_dx}/{ld_y} lead {lead_dx}/{lead_y}"
    assert (got[:, cols:] == SENTINEL).all(), "a gap column of dx was written"
    assert np.array_equal(yb.bits(), _bits(yf).reshape(-1)), "y was written"
    return db, yb


@pytest.mark.parametrize("rows,cols", [(8, 64), (300, 512)])
def test_relu_backward_dense_aligned(rows, cols):
    """Dense, 16-byte aligned, rows * cols a multiple of 4: the float4 form (relu_backward4_kernel), one block and many.

    Bit-identical to ``torch.where(y > 0, dx, 0)`` in all four forms.  y holds no NaN: the kernel zeroes the gradient where y is
    NaN (it tests ``!(y > 0)``) while torch's ``threshold_backward`` passes it; the difference is known and deliberate, and
    unreachable in a live run, where y is the output of a ReLU."""
    db, yb = _relu_case(rows, cols, cols, cols)
    assert db.t.data_ptr() % 16 == 0 and yb.t.data_ptr() % 16 == 0 and (rows * cols) % 4 == 0          # the form's conditions


@pytest.mark.parametrize("rows,cols", [(3, 5), (7, 9)])
def test_relu_backward_dense_total_not_a_multiple_of_4(rows, cols):
    """Dense and aligned but rows * cols % 4 != 0: the scalar form; the float4 form would read and write past the end."""
    assert (rows * cols) % 4 != 0
    _relu_case(rows, cols, cols, cols)


@pytest.mark.parametrize("lead_dx,lead_y", [(GUARD + 1, GUARD + 1), (GUARD + 1, GUARD), (GUARD, GUARD + 1)], ids=["both", "dx", "y"])
def test_relu_backward_dense_unaligned_base(lead_dx, lead_y):
    """Dense, total a multiple of 4, but dx and / or y start one float into an aligned buffer: the scalar form."""
    db, yb = _relu_case(8, 64, 64, 64, lead_dx, lead_y)
    assert (db.t.data_ptr() % 16 != 0) == (lead_dx != GUARD) and (yb.t.data_ptr() % 16 != 0) == (lead_y != GUARD)


@pytest.mark.parametrize("rows,cols", [(20, 512), (300, 90)])
def test_relu_backward_strided(rows, cols):
    """ld_dx = cols + 6, ld_y = cols + 2 (as HeadTrainer calls it, where dY is padded to the GEMM's column stride): the strided
    scalar form; the six gap columns of every dx row stay untouched."""
    _relu_case(rows, cols, cols + 6, cols + 2)


def test_relu_backward_refuses_null_and_empty():
    L, st = _lib()
    b = _Buf(64).put(np.ones(64))
    assert L.ihmr_relu_backward(None, b.ptr(), 8, 8, 8, 8, st) != 0
    assert L.ihmr_relu_backward(b.ptr(), None, 8, 8, 8, 8, st) != 0
    assert L.ihmr_relu_backward(b.ptr(), b.ptr(), 0, 8, 8, 8, st) != 0
    assert L.ihmr_relu_backward(b.ptr(), b.ptr(), 8, 0, 8, 8, st) != 0
    torch.cuda.synchronize()
    assert (b.bits() == _bits(np.ones(1))[0]).all()
