#!/usr/bin/env python
"""microbenchmark of the fused update-operator chains at the bench size (HIP events, 50 launches each)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from rampvo_amd.synthetic import make_network
E = int(sys.argv[1]) if len(sys.argv) > 1 else 40000
net = make_network("SingleScale")
fu = net.update.fused(torch.float16)
g = torch.Generator().manual_seed(1)
rnd = lambda *s: (torch.randn(*s, generator=g) * 0.5).cuda()
x32, hy = rnd(E, 384), rnd(2200, 384).half()
gid = torch.randint(0, 2200, (E,), generator=g).int().cuda()
idx = (torch.arange(E) - 1).cuda() if os.environ.get("MB_ADJ") else torch.randint(-1, E, (E,), generator=g).cuda()
if os.environ.get("MB_ADJ"):
    gid = (torch.arange(E) // 19).int().cuda()
corr = F.pad(rnd(E, 882).half(), (0, 14)).contiguous()
net_map = torch.randint(-1, E, (E,), generator=g).cuda()
table = rnd(3072, 384).half(); inp_idx = torch.randint(0, 100000, (E,), generator=g).cuda()
gru = lambda: fu.gru(x32, add=(hy, gid))
nbr = lambda: fu.nbr(x32, idx, "c1")
corr_mlp = lambda: fu.corr_mlp(corr, x32, net_map, table, inp_idx, 3072)
fgk = lambda: fu.fg(x32, hy, gid, fu.weights()["kk_fg_pack"], E, write_back=False)
res = {}
for name, fn in (("gru", gru), ("nbr", nbr), ("corr_mlp", corr_mlp), ("fg", fgk)):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(50):
        fn()
    e.record(); torch.cuda.synchronize()
    res[name] = s.elapsed_time(e) / 50 * 1e3
print("E=%d RAMP_UPD_BIG=%s: " % (E, os.environ.get("RAMP_UPD_BIG", "auto")) + "  ".join("%s %.1f us" % kv for kv in res.items()), flush=True)
