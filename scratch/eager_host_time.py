"""python scratch/eager_host_time.py TREE [tiny]: host time of 20 eager c5 training steps (cfg.HIP.TRAIN_REPLAY off) on TREE's code, on a 160 x 224
image (the same layers and launches as full size, a few ms of GPU work: the step is bound by the host's enqueue) and at full size; `tiny`: the small image three times."""
import os
import sys
import time

tree = os.path.abspath(sys.argv[1])
sys.path.insert(0, tree)
import bench  # noqa: E402
import torch  # noqa: E402
from frcnn_hip.runtime import Session  # noqa: E402
from model.config import cfg  # noqa: E402
from model.train_val import SolverWrapper, synthetic_data_layer  # noqa: E402

assert os.path.dirname(os.path.abspath(bench.__file__)) == tree
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO, cfg.TRAIN.DOUBLE_BIAS = 256, 0.0, False
cfg.HIP.MFMA_H2 = cfg.HIP.MFMA_X3 = True
cfg.HIP.TRAIN_REPLAY = False
c = bench.CONFIGS["c5"]
for h, w in (((160, 224), (600, 1000)) if len(sys.argv) < 3 else ((160, 224),) * 3):
    sess = Session(device=dev, seed=cfg.RNG_SEED)
    net = bench.make_net(c)
    net.create_architecture("TRAIN", c["classes"], tag="eh%d" % h, anchor_scales=c["scales"], anchor_ratios=bench.ANCHOR_RATIOS)
    sess.init_variables(net.variable_specs())
    layer = bench.resident_blobs(synthetic_data_layer(c["classes"], seed=3, height=h, width=w, scale=1.0, image_gain=1 / 256.0), dev)
    sw = SolverWrapper(sess, net, layer)
    sw.train_model(5, verbose=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sw.train_model(20, verbose=False)
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    assert net.replay_stats == dict(eager=0, recorded=0, replayed=0), net.replay_stats
    print("%dx%d host_ms_per_step %.3f completed_ms_per_step %.3f" % (h, w, 1e3 * host / 20, 1e3 * total / 20), flush=True)
    sess.close()
