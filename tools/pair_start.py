"""Start-up of the stream-K pair kernel: the time a wave spends between kernel entry and the moment its first operand
requests have been issued (the stream-K cut, the segment decode, the operand addresses), for wave 0 and for the last wave of
the launch, in a sustained H = 40 loop at C2 (tools/pair_clock.py: a short run reads a lower clock).  Needs a library built
with EXTRA=-DPAIR_START_STAMP (named by PILCO_LIB); stamps are 100 MHz wall-clock ticks, so single readings step by 10 ns."""
import numpy as np, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pilco_amd import _lib, synthetic
cfg = synthetic.config_c2(N=1000, D=10, E=10)
ctx = _lib.Context()
ctx.debug_timestamps(read=False)
ctx.gp_set_data(0, cfg["X"], cfg["Y"]); ctx.gp_set_hyp(0, cfg["lengthscales"], cfg["variance"], cfg["noise"]); ctx.gp_factorize(0)
pol = dict(kind=_lib.POLICY_NONE, state_dim=10, control_dim=0)
rw = [dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=np.eye(10), t=np.zeros(10))]
for _ in range(10):
    ctx.rollout(pol, rw, cfg["m0"], cfg["S0"], 40)
first, last, dur = [], [], []
for rep in range(40):
    ctx.rollout(pol, rw, cfg["m0"], cfg["S0"], 40)     # (eager with stamps: the LAST step's pair launch is what the stamps hold)
    ts = ctx.debug_timestamps()
    if ts[46] > ts[16] and ts[39] > ts[38]:
        first.append((ts[46] - ts[16]) / 100.0)
        last.append((ts[39] - ts[38]) / 100.0)
        dur.append((ts[17] - ts[16]) / 100.0)
if not first:
    sys.exit("%s holds no start-up stamps: build it with EXTRA=-DPAIR_START_STAMP" % os.path.basename(_lib.LIB_PATH))
print("%s pair start-up, entry -> first operand requests issued (us): wave 0 mean %.3f median %.2f min %.2f max %.2f | last wave mean %.3f median %.2f min %.2f max %.2f | wave 0 runs %.1f us | %d launches" % (
    os.path.basename(_lib.LIB_PATH), np.mean(first), np.median(first), min(first), max(first),
    np.mean(last), np.median(last), min(last), max(last), np.median(dur), len(first)))
ctx.close()
