#!/usr/bin/env python
"""microbenchmark of the fp32-accuracy update-operator chains (csrc/update_x3.hip) at the bench size (HIP events, 30 launches
each), next to the library-GEMM operator they replace (RAMP_X3=0's path) -- tools/mb_update.py is the fp16 twin"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from types import SimpleNamespace
from rampvo_amd.synthetic import make_network
E = int(sys.argv[1]) if len(sys.argv) > 1 else 40000
net = make_network("SingleScale")
fu = net.update.fused(torch.float32)
w = fu.weights()
g = torch.Generator().manual_seed(1)
rnd = lambda *s: (torch.randn(*s, generator=g) * 0.5).cuda()
G = 2200
x32, h0, h1 = rnd(E, 384), rnd(G, 384), rnd(G, 384)
gid = (torch.arange(E) // 19).int().cuda() % G
order = torch.argsort(gid.long(), stable=True).int()
seg = torch.zeros(G + 1, dtype=torch.int32, device="cuda")
seg[1:] = torch.cumsum(torch.bincount(gid.long(), minlength=G), 0).int()
grp = SimpleNamespace(order=order, seg_start=seg, ngroups=torch.tensor([G], dtype=torch.int32, device="cuda"))
out32 = torch.empty(E, 384, device="cuda")
idx = (torch.arange(E) - 1).cuda()
corr = F.pad(rnd(E, 882), (0, 14)).contiguous()
net_map = torch.randint(-1, E, (E,), generator=g).cuda()
table = rnd(3072, 384); inp_idx = torch.randint(0, 100000, (E,), generator=g).cuda()
coords = (torch.rand(E, 2, 3, 3, generator=g) * 60).cuda()
gru = lambda: fu.gru(x32, add=(h1, gid), add0=(h0, gid), heads_at=(coords, 160.0, 120.0))
nbr = lambda: fu.nbr(x32, idx, "c1")
corr_mlp = lambda: fu.corr_mlp(corr, x32, net_map, table, inp_idx, 3072)
fgk = lambda: fu.fg(x32, h0, gid, w["kk_fg_pack"], E, write_back=False)
fg = fgk()
segk = lambda: fu.seg(fg, grp, G)
y = segk()
lin = lambda: fu.h_lin(y, w["kk_h_pack"], grp)
def lib_gemm():                      # one [E,384] x [384,384] fp32 library GEMM: what a layer of RAMP_X3=0's path costs
    torch.mm(x32, w["c1a"][0].t(), out=out32)
res = {}
for name, fn in (("gru+heads", gru), ("nbr", nbr), ("corr_mlp", corr_mlp), ("fg", fgk), ("segsoftmax", segk), ("h", lin),
                 ("torch.mm fp32 (1 layer)", lib_gemm)):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(30):
        fn()
    e.record(); torch.cuda.synchronize()
    res[name] = s.elapsed_time(e) / 30 * 1e3
op = res["corr_mlp"] + 2 * res["nbr"] + 2 * (res["fg"] + res["segsoftmax"] + res["h"]) + res["gru+heads"]
print("E=%d x3: " % E + "  ".join("%s %.1f us" % kv for kv in res.items()) + "  | operator %.0f us = %.0f TFLOP/s fp32-equivalent"
      % (op, E * 5.4e6 / op / 1e6), flush=True)
