"""Device buffers between guard regions, and an `OptimizeModel` moved onto them.  Importing this module touches no GPU.

`Guarded(nbytes)`: ONE ordinary allocation `guard | payload | guard`, the payload exactly `nbytes` long and starting at a 256-aligned
address, the guards filled with 0xA5, the payload with a chosen byte.  A kernel that stores a few bytes -- or a whole hand's record --
past either end of the buffer it was handed damages a guard and `guards_intact()` names the first damaged byte; a kernel that reads a
region nobody has written reads the fill, so two runs with different fills differ.  (The generalisation of `_Buf` of
tests/test_gpu_mano_layer.py.)

Guard widths: `WORKSPACE_GUARD` on each side of a workspace -- at least one hand's largest region, its candidate lists
`SDF_LCAP_V * SDF_LCAP_L * 2` = 393 216 bytes (tests/test_workspace_carve_cpu.py derives that from the carve tables), so an overrun by
one hand's record of any region lands in a guard; `SMALL_GUARD` = 4 KiB around the small per-sample buffers."""
import torch

GUARD_BYTE = 0xA5
SMALL_GUARD = 4096
WORKSPACE_GUARD = 1024 * 192 * 2 + 4096       # one hand's candidate lists and a page
ALIGN = 256
FILLS = (0x00, 0xFF, 0xA5)                    # 0xFF: counters of -1 and NaN floats; 0xA5: large indices


class Guarded:
    def __init__(self, nbytes, guard=SMALL_GUARD, fill=GUARD_BYTE, device="cuda"):
        assert nbytes >= 0 and guard > 0
        self.nbytes, self.guard = int(nbytes), int(guard)
        self.raw = torch.full((self.guard + ALIGN + self.nbytes + self.guard,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.lo = self.guard + (-(self.raw.data_ptr() + self.guard)) % ALIGN       # payload offset in `raw`
        self.payload = self.raw[self.lo:self.lo + self.nbytes]
        assert self.payload.data_ptr() % ALIGN == 0 or self.raw.device.type != "cuda" or self.nbytes == 0
        self.fill(fill)

    def fill(self, byte):
        self.payload.fill_(int(byte))
        return self

    @property
    def data_ptr(self):
        return self.raw.data_ptr() + self.lo

    def payload_bytes(self):
        """The payload as a uint8 tensor (a view: what a kernel wrote is visible here)."""
        return self.payload

    def view(self, dtype, shape):
        """The payload as a tensor of `dtype` and `shape` (a view; the shape must fill the payload exactly)."""
        t = self.payload.view(dtype).view(shape)
        assert t.numel() * t.element_size() == self.nbytes
        return t

    def copy_in(self, src):
        """Fill the payload with the bytes of `src` (a contiguous tensor of exactly `nbytes`); returns the view of its dtype and shape."""
        v = self.view(src.dtype, src.shape)
        v.copy_(src)
        return v

    def guards_intact(self):
        """None if both guards still hold GUARD_BYTE everywhere, else the payload-relative offset of the first damaged byte (negative:
        in front of the payload; >= nbytes: behind it)."""
        hi = self.lo + self.nbytes
        for start, part in ((0, self.raw[:self.lo]), (hi, self.raw[hi:])):
            bad = part != GUARD_BYTE
            if bool(bad.any().item()):
                return start + int(bad.int().argmax().item()) - self.lo
        return None


def assert_guards(buffers, when=""):
    """`buffers`: name -> Guarded.  Fails with the buffer and the first damaged offset (look the offset up in the carve table that
    tests/test_workspace_carve_cpu.py prints)."""
    for name, g in buffers.items():
        off = g.guards_intact()
        assert off is None, f"{when}: guard of `{name}` ({g.nbytes} bytes) damaged at payload offset {off}"


def guard_model(model, fill=GUARD_BYTE, workspace=None):
    """Move every buffer of an `OptimizeModel` into a guarded allocation of exactly `numel * itemsize` bytes: inputs, state and outputs
    are copied in, the workspace is filled with `fill` (or is `workspace`, a Guarded some other model already uses, at least as large).
    The views replace the entries of `model.buf`, the addresses the same-named pointer fields of `model.io`.  Captured graphs bake the
    addresses in, so this has to happen before the first capture.  Returns name -> Guarded."""
    assert not model._graphs, "guard_model() after a graph was captured: the graph holds the old addresses"
    out = {}
    for name, t in list(model.buf.items()):
        nbytes = t.numel() * t.element_size()
        if name == "workspace":
            g = workspace if workspace is not None else Guarded(nbytes, guard=WORKSPACE_GUARD, fill=fill, device=t.device)
            assert g.nbytes >= nbytes
            view = g.payload[:nbytes]
        else:
            assert t.is_contiguous()
            g = Guarded(nbytes, guard=SMALL_GUARD, device=t.device)
            view = g.copy_in(t)
        assert hasattr(model.io, name), name
        model.buf[name] = view
        setattr(model.io, name, g.data_ptr)
        out[name] = g
    return out
