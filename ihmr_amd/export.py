"""The result export of the three models (``get_pred_result`` / ``get_pred_result_async``): one exporter, one handle.

The contract, stated once for ``OptimizeModel``, ``MLPModel`` and ``InterHandModel``:

* the transfer is ONE gather launch (``ihmr_copy_segments``) into a device pack buffer plus ONE device-to-host copy into pinned memory;
* the asynchronous handle returns VIEWS of a two-slot pinned ring: valid until the next-but-one export of that exporter, blocking ones counted;
* the blocking export returns arrays the caller OWNS: the reference's loops keep every batch's rows until they pickle them at the end
  (``optimize.py:61-71``, ``test_mlp.py:61-68``; ``evaluator.py:38-97`` stores row views).
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch

from . import hip


class PendingResult:
    """Handle of an export in flight: the pinned buffer and where every key lies in it (``key -> (offset, shape, dtype, bytes)``), the
    event recorded behind the copy, the constant keys made on the host (``key -> value``: int32, one entry per sample) and the order
    in which the keys are handed out."""

    def __init__(self, host, layout, event, host_keys, order, batch_size):
        self._host, self._layout, self._event = host, layout, event
        self._host_keys, self._order, self._n = host_keys, order, batch_size

    def wait(self):
        self._event.synchronize()
        out = {k: np.full(self._n, value, dtype=np.int32) for k, value in self._host_keys.items()}
        for k, (o, shape, dt, nbytes) in self._layout.items():
            out[k] = self._host[o:o + nbytes].view(dt).view(shape).numpy()
        return OrderedDict((k, out[k]) for k in self._order)


class ResultExporter:
    """The export state of one model instance: the cached layout (``_layout``: the key under which the buffers below were allocated; a
    change of any key's shape or dtype replaces all three), ONE device pack buffer and the two-slot pinned ring with the slot last
    written.  One pack buffer serves both slots only because gather and device-to-host copy are queued on the same stream, the
    caller's current one: the next gather cannot overtake the copy before it.  Export one instance from one stream."""

    def __init__(self, device):
        self.device = device
        self._layout, self._pack, self._pinned, self._slot = None, None, [None, None], 0

    def start(self, sources, host_keys, order):
        """``sources``: key -> device tensor with one row per sample, or a tuple of 2-D tensors that the export lays side by side (the
        columns of one array, as ``torch.cat(..., dim=1)`` would, without that kernel).  Queued on the current stream, behind what
        produced the values."""
        sources = OrderedDict((k, tuple(t.detach() for t in (v if isinstance(v, tuple) else (v,)))) for k, v in sources.items())
        layout, off, n = OrderedDict(), 0, next(iter(sources.values()))[0].shape[0]
        for k, parts in sources.items():
            assert all(p.dim() >= 1 and p.shape[0] == n for p in parts), f"{k}: every source has one row per sample ({n})"
            shape = tuple(parts[0].shape) if len(parts) == 1 else (parts[0].shape[0], sum(p.shape[1] for p in parts))
            nbytes = int(np.prod(shape)) * parts[0].element_size()
            layout[k] = (off, shape, parts[0].dtype, nbytes)
            off += (nbytes + 15) // 16 * 16
        if layout != self._layout:               # first export, or a source changed shape or dtype: earlier handles keep the old buffers
            self._layout = layout
            self._pack = torch.empty(off, dtype=torch.uint8, device=self.device)
            self._pinned = [torch.empty(off, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self._slot ^= 1
        pairs = []
        for k, parts in sources.items():
            o, shape, dt, nbytes = layout[k]
            dst = self._pack[o:o + nbytes].view(dt).view(shape)
            for v, d in zip(parts, (dst,) if len(parts) == 1 else dst.split([p.shape[1] for p in parts], dim=1)):
                if v.element_size() not in (4, 8):
                    d.copy_(v)                   # ihmr_copy_segments moves dwords
                    continue
                if not (v.is_contiguous() or (v.dim() == 2 and v.stride(1) == 1)):    # (a column slice goes in as a strided segment)
                    v = v.contiguous()
                pairs.append((v, d))
        hip.copy_segments(pairs)
        host = self._pinned[self._slot]
        host.copy_(self._pack, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        return PendingResult(host, layout, event, host_keys, order, n)

    def blocking(self, sources, host_keys, order):
        return OrderedDict((k, np.array(v, copy=True)) for k, v in self.start(sources, host_keys, order).wait().items())
