"""The workload of the scaled-decode counter passes: 64 x 4096^2 L4 grids decoded at s = 1 and s = 2, five launches each
(after one checked warm-up), nothing else on the device.  Run under rocprofv3 with ONE --pmc counter per pass, e.g.
  rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d out/fetch -- python3 tools/scaled_prof.py
  rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d out/write -- python3 tools/scaled_prof.py
and read the k_dec_scaled rows: bytes = 2 * FETCH_SIZE * 1024 (gfx950 counts half of a wide streaming read) and
WRITE_SIZE * 1024 (profiles/r06_scaled.txt)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rustyhgi_amd as H  # noqa: E402
from rustyhgi_amd import _ffi  # noqa: E402

L = _ffi.lib()
ctx = H.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
w = h = 4096
B, levels = 64, 4
grid = torch.empty((B, h, w), dtype=torch.uint8, device="cuda")
_ffi.check(L.hgi_synth_u8_dev(ctx.handle, _ffi.SYNTH_NOISE, 0x48474934, 0, w, h, grid.data_ptr(), B, w * h))
full = torch.empty_like(grid)
_ffi.check(L.hgi_decode_u8_dev(ctx.handle, grid.data_ptr(), w, h, levels, 1, full.data_ptr(), B, w * h))
for s in (1, 2):
    sw, sh = w >> s, h >> s
    out = torch.empty((B, sh, sw), dtype=torch.uint8, device="cuda")
    for _ in range(6):
        _ffi.check(L.hgi_decode_scaled_u8_dev(ctx.handle, grid.data_ptr(), w, h, levels, 1, s, out.data_ptr(), sw, B, w * h, sw * sh))
    torch.cuda.synchronize()
    assert torch.equal(out, full[:, ::1 << s, ::1 << s]), s
ctx.close()
print("scaled_prof ok")
