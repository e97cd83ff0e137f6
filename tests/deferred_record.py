"""node_step_record (include/node_hip.h) as a deferred solve leaves it in device memory, for the tests that read it directly."""
import ctypes as C

import torch

RECORD_BYTES = 128       # what the tests allocate; the struct is smaller


def new_record(device='cuda'):
    return torch.zeros(RECORD_BYTES, dtype=torch.uint8, device=device)


def read_record(rec_bytes):
    """dict of the record's fields, through the binding's own structure (no offsets restated here)."""
    from neural_ode_features_amd import _lib
    raw = bytes(rec_bytes.cpu().tolist())
    st = _lib.NodeStepRecord.from_buffer_copy(raw[:C.sizeof(_lib.NodeStepRecord)])
    return {name: getattr(st, name) for name, _ in _lib.NodeStepRecord._fields_}
