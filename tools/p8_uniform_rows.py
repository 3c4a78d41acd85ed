"""Does conv_igemm_p8's time follow its K-tiles?  3x3 convs through cbw_conv2d whose tiles all drop the same kernel rows
under CBW_P8_ROWSKIP -- Ho 1 walks 3 of 9 taps, Ho 2 6 of 9 -- beside mixed ones (Ho 3, Ho 5) at the same ~4.5 rounds
of 256 x 256 tiles; switch off / on alternating, best of 4 rounds of 10 (profiles/rowskip_layers_ab.txt section 3)."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "enhance-cb-whisper_amd")]
from cbw import _lib  # noqa: E402

lib = _lib.load()
d = torch.device("cuda:0")
for (N, H, W, C) in [(6144, 1, 24, 512), (3072, 2, 24, 512), (2048, 3, 24, 512), (6144, 1, 47, 256), (3072, 2, 47, 256),
                     (1229, 5, 47, 256)]:
    x = torch.randn((N, H, W, C), device=d).to(torch.bfloat16)
    w = (torch.randn((C, 3, 3, C), device=d) / (9 * C) ** 0.5).to(torch.bfloat16)
    b = torch.randn(C, device=d)
    y = torch.empty((N, H, W, C), device=d, dtype=torch.bfloat16)
    args = (x.data_ptr(), w.data_ptr(), b.data_ptr(), None, y.data_ptr(), N, H, W, C, C, 3, 3, 1, 1, 1, 1, 1,
            _lib.stream_handle())
    ts = {}
    for rnd in range(4):
        for mode in (("0", "1") if rnd % 2 == 0 else ("1", "0")):
            os.environ["CBW_P8_ROWSKIP"] = mode
            lib.cbw_conv2d(*args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                lib.cbw_conv2d(*args)
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1) / 10 * 1e3
            ts[mode] = min(ts.get(mode, t), t)
    tiles = (N * H * W + 255) // 256 * (C // 256)
    print(f"N {N} H {H} W {W} C {C}: {tiles} tiles ({tiles / 256:.2f} rounds)  off {ts['0']:.1f} us  on {ts['1']:.1f} us  "
          f"on/off {ts['1'] / ts['0']:.3f}", flush=True)
