"""python scratch/dump_train_recording.py TREE OUT: three c5 training steps (eager, recorded, replayed) on TREE's code; writes the recorded
step (Recording.cmds) to OUT: per command the entry name, the stream slot and the non-pointer scalar arguments; OP entries as their position."""
import ctypes
import os
import sys

tree, out = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, tree)
import bench  # noqa: E402
import torch  # noqa: E402
from frcnn_hip import replay  # noqa: E402
from frcnn_hip.runtime import Session  # noqa: E402
from frcnn_hip.train import TrainState  # noqa: E402
from model.config import cfg  # noqa: E402
from model.train_val import synthetic_data_layer  # noqa: E402

assert os.path.dirname(os.path.abspath(bench.__file__)) == tree
dev = torch.device("cuda", 0)
c = bench.CONFIGS["c5"]
cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO, cfg.TRAIN.DOUBLE_BIAS = 256, 0.0, False
cfg.HIP.MFMA_H2 = cfg.HIP.MFMA_X3 = True
cfg.HIP.TRAIN_REPLAY = True
sess = Session(device=dev, seed=cfg.RNG_SEED)
net = bench.make_net(c)
net.create_architecture("TRAIN", c["classes"], tag="c5dump", anchor_scales=c["scales"], anchor_ratios=bench.ANCHOR_RATIOS)
sess.init_variables(net.variable_specs())
ts = TrainState(sess, net, momentum=cfg.TRAIN.MOMENTUM, weight_decay=cfg.TRAIN.WEIGHT_DECAY)
ts.lr = 1e-3
ledger = ts.flop_ledger = {}
layer = synthetic_data_layer(c["classes"], seed=cfg.RNG_SEED, image_gain=1 / 256.0)
blob = next(layer)
losses, ledgers = [], []
for i in range(3):
    ledger.clear()
    losses.append([float(v) for v in net.train_step(sess, blob, ts)])
    ledgers.append(sorted(ledger.items()))
torch.cuda.synchronize()
recs = [ent.rec for ent in sess.graphs.values() if isinstance(ent, replay.RecordedStep) and ent.rec is not None]
assert len(recs) == 1 and net.replay_stats == dict(eager=1, recorded=1, replayed=1), net.replay_stats
rec = recs[0]
POINTERS = (ctypes.c_void_p, ctypes.c_char_p, ctypes._Pointer, ctypes.Array)
with open(out, "w") as f:
    for i, cmd in enumerate(rec.cmds):
        if cmd[0] == rec.OP:
            f.write("OP %d\n" % i)
            continue
        _, fn, conv, si, slot, name = cmd
        scalars = [repr(a.value) if isinstance(a, ctypes._SimpleCData) else repr(a) for a in conv if not isinstance(a, POINTERS)]
        f.write("%s slot=%d %s\n" % (name, slot, " ".join(scalars)))
    f.write("n_calls %d cmds %d streams %d flops %r\n" % (rec.n_calls, len(rec.cmds), len(rec.streams), ledgers[1]))
    f.write("losses %r\n" % (losses,))
print("%s: cmds %d n_calls %d streams %d" % (out, len(rec.cmds), rec.n_calls, len(rec.streams)))
