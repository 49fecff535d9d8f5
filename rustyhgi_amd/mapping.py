"""Tables of `Decoder.decode_mapped` (include/hgi_map.h): 256 output elements, one per value of a decoded pixel -- and the
constants of `Encoder.encode_typed` (include/hgi_typed.h) that take such frames back to pixels.

The codec moves the table's bits and does no float arithmetic, so whatever conversion a pipeline wants -- x / 255, mean / std
normalisation, gamma -- is computed here, once, on the host or by torch, and never repeated by the library.
"""
import numpy as np


def _is_torch_dtype(dtype):
    return type(dtype).__module__.startswith("torch")


def affine_table(dtype, scale=1.0 / 255.0, bias=0.0, device=None):
    """`(arange(256, float32) * scale + bias).to(dtype)`: the table that maps pixel v to v * scale + bias (default: v / 255).
    The arithmetic is float32, rounded once to `dtype`.  A numpy dtype (float16, float32, ...) gives a numpy array -- or, with
    `device`, a torch tensor there; a torch dtype (torch.bfloat16 has no numpy counterpart) gives a torch tensor on `device`
    (default: the CPU).  The hot path keeps the table on the frames' device and passes that tensor to every call."""
    if _is_torch_dtype(dtype):
        import torch
        t = (torch.arange(256, dtype=torch.float32) * torch.tensor(scale, dtype=torch.float32)
             + torch.tensor(bias, dtype=torch.float32)).to(dtype)
        return t if device is None else t.to(device)
    tab = (np.arange(256, dtype=np.float32) * np.float32(scale) + np.float32(bias)).astype(np.dtype(dtype))
    if device is None:
        return tab
    import torch
    return torch.from_numpy(tab).to(device)


def affine_inverse(scale=1.0 / 255.0, bias=0.0):
    """The `(scale, bias)` of `Encoder.encode_typed` that invert `affine_table(dtype, scale, bias)`: float32
    `(1 / scale, -bias / scale)`, so that `x * (1 / scale) + (-bias / scale)` rounds back to the pixel v that the table mapped
    to x = v * scale + bias.  Both quotients are float32 divisions of the float32 arguments."""
    s, b = np.float32(scale), np.float32(bias)
    return np.float32(1) / s, -b / s
