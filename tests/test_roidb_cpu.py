"""CPU: the training roidb and data layer (datasets.pascal_voc.gt_roidb, datasets.imdb.append_flipped_images, roi_data_layer,
model.train_val.get_training_roidb / filter_roidb, the snapshot's data-layer state) against tests/golden/roidb.npz, which
fixtures/gen_golden_roidb.py produced by running the REFERENCE's own modules on the same seeded devkit."""
import json
import os
import pickle
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import gen_golden_roidb as ggr  # noqa: E402  (test infrastructure: devkit builder + fixture layout)


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "roidb.npz")))


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("voc_data"))
    ggr.build_devkit(d)
    return d


def draw(layer, n):
    """n minibatches -> (db_inds, scale_inds, im_info [n,3], gt_boxes list)"""
    db, sc, info, gt = [], [], [], []
    for _ in range(n):
        blobs = layer.forward()
        db.append(layer.last_draw[0])
        sc.append(layer.last_draw[1])
        info.append(blobs["im_info"])
        gt.append(blobs["gt_boxes"])
    return np.array(db, dtype=np.int64), np.array(sc, dtype=np.int64), np.stack(info), gt


@pytest.mark.parametrize("flipped", [True, False])
def test_roidb_fields_and_filter_equal_the_reference(fixture, data_dir, flipped):
    with ggr.repo_cfg(data_dir, flipped=flipped):
        imdb, roidb, filtered = ggr.repo_roidb()
    want = {}
    ggr.roidb_arrays(ggr.case_prefix(flipped), roidb, want)
    keys = [k for k in fixture if k.startswith(ggr.case_prefix(flipped) + "e") or k == ggr.case_prefix(flipped) + "n"]
    assert sorted(want) == sorted(keys) and len(roidb) == (14 if flipped else 7) == imdb.num_images
    for k in keys:
        assert want[k].dtype == fixture[k].dtype and want[k].shape == fixture[k].shape and np.array_equal(want[k], fixture[k]), k
    assert roidb[0]["boxes"].dtype == np.uint16 and roidb[0]["gt_classes"].dtype == np.int32 and roidb[0]["seg_areas"].dtype == np.float32
    kept = [k for k, e in enumerate(roidb) if any(e is f for f in filtered)]
    assert kept == fixture[ggr.case_prefix(flipped) + "filtered"].tolist()
    # the image whose objects are all `difficult` has no box without use_diff: it and its mirrored twin are dropped
    assert ggr.ALL_DIFFICULT not in kept and (not flipped or ggr.ALL_DIFFICULT + 7 not in kept) and len(kept) == (12 if flipped else 6)
    assert imdb.num_classes == 21 and imdb.name == "voc_2007_trainval" and imdb.image_path_at(0).endswith("000001.jpg")


def test_use_diff_keeps_difficult_objects_and_unknown_methods_raise(data_dir):
    from datasets.factory import get_imdb
    with ggr.repo_cfg(data_dir):
        plain, diff = get_imdb("voc_2007_trainval"), get_imdb("voc_2007_trainval_diff")
        assert diff.name == "voc_2007_trainval_diff"
        assert len(plain.roidb[ggr.ALL_DIFFICULT]["boxes"]) == 0 < len(diff.roidb[ggr.ALL_DIFFICULT]["boxes"])
        _, objects = ggr.synth_devkit_arrays()
        assert [len(e["boxes"]) for e in diff.roidb] == [len(o) for o in objects]
        o = objects[0][0]
        assert diff.roidb[0]["boxes"][0].tolist() == [o[1] - 1, o[2] - 1, o[3] - 1, o[4] - 1]          # 1-based -> 0-based
        with pytest.raises(NotImplementedError):
            plain.set_proposal_method("selective_search")
        with pytest.raises(KeyError):
            get_imdb("coco_2014_train")


@pytest.mark.parametrize("grouping", [False, True])
@pytest.mark.parametrize("flipped", [True, False])
def test_minibatch_sequence_equals_the_reference(fixture, data_dir, flipped, grouping):
    from roi_data_layer.layer import RoIDataLayer
    gp = ggr.case_prefix(flipped, grouping)
    with ggr.repo_cfg(data_dir, flipped=flipped, grouping=grouping):
        imdb, _, filtered = ggr.repo_roidb()
        np.random.seed(ggr.SEED)
        layer = RoIDataLayer(filtered, imdb.num_classes)
        n = ggr.n_draws(len(filtered))
        db, sc, info, gt = draw(layer, n)
        after = np.random.rand()
    assert n == len(fixture[gp + "db_inds"]) >= 2.5 * len(filtered)
    assert np.array_equal(db, fixture[gp + "db_inds"]) and np.array_equal(sc, fixture[gp + "scale_inds"])
    assert info.dtype == np.float32 and np.array_equal(info, fixture[gp + "im_info"])
    for k in range(n):
        assert gt[k].dtype == np.float32 and gt[k].shape == fixture["%sgt%d" % (gp, k)].shape and np.array_equal(gt[k], fixture["%sgt%d" % (gp, k)]), k
    assert after == float(fixture[gp + "rand_after"])                      # the same amount of the global stream was consumed
    assert len(set(sc.tolist())) == 2                                      # both scales occur: the randint matters


def test_raw_image_blob_form(data_dir):
    from roi_data_layer.layer import RoIDataLayer
    with ggr.repo_cfg(data_dir):
        imdb, _, filtered = ggr.repo_roidb()
        np.random.seed(ggr.SEED)
        layer = RoIDataLayer(filtered, imdb.num_classes)
        blobs = next(layer)
        images, _ = ggr.synth_devkit_arrays()
    e = filtered[layer.last_draw[0]]
    assert "data" not in blobs and blobs["image"].dtype == np.uint8 and blobs["image"].shape == (e["height"], e["width"], 3)
    assert np.array_equal(blobs["image"], images[int(os.path.basename(e["image"])[:6]) - 1][:, :, ::-1])      # BGR, NOT mirrored on the host
    assert blobs["flipped"] == e["flipped"] and blobs["target_size"] == ggr.SCALES[layer.last_draw[1]] and blobs["max_size"] == ggr.MAX_SIZE
    assert blobs["boxes"].dtype == np.uint16 and blobs["gt_classes"].dtype == np.int32 and len(blobs["boxes"]) == len(blobs["gt_boxes"])


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("grouping", [False, True])
def test_ranks_partition_the_single_rank_sequence(fixture, data_dir, world, grouping):
    from roi_data_layer.layer import RoIDataLayer
    gp = ggr.case_prefix(True, grouping)
    want = list(zip(fixture[gp + "db_inds"].tolist(), fixture[gp + "scale_inds"].tolist()))
    per = len(want) // world
    got = [None] * (per * world)
    with ggr.repo_cfg(data_dir, grouping=grouping):
        imdb, _, filtered = ggr.repo_roidb()
        for rank in range(world):
            np.random.seed(ggr.SEED)                                      # every rank: the same seed, the same roidb
            layer = RoIDataLayer(filtered, imdb.num_classes, rank=rank, world_size=world)
            db, sc, _, _ = draw(layer, per)
            got[rank::world] = list(zip(db.tolist(), sc.tolist()))
    assert got == want[:per * world]                                      # rank r holds draws r, r+W, ...: the union is the W = 1 sequence, in order


def _solver(layer):
    """A SolverWrapper over the host half of a session (no GPU): enough for snapshot() / restore()."""
    from frcnn_hip.runtime import VariableStore
    from model.train_val import SolverWrapper
    sess = VariableStore(seed=1)
    sess.variables["v/weights"] = np.arange(6, dtype=np.float32).reshape(2, 3)
    sess.prepared = types.SimpleNamespace(invalidate=lambda: None)
    return SolverWrapper(sess, types.SimpleNamespace(_sample_seed=10), layer)


def _resume_child(data_dir, sfile, nfile, n, world, rank):
    """(runs in a fresh interpreter) a new layer over a new roidb, restored from the snapshot: prints its next n draws"""
    from roi_data_layer.layer import RoIDataLayer
    with ggr.repo_cfg(data_dir):
        imdb, _, filtered = ggr.repo_roidb()
        np.random.seed(12345)                                             # a state of its own: restore() must replace it
        layer = RoIDataLayer(filtered, imdb.num_classes, rank=rank, world_size=world)
        sw = _solver(layer)
        it = sw.restore(sfile, nfile)
        db, sc, _, _ = draw(layer, n)
    print("RESUMED " + json.dumps(dict(iter=it, seed=sw.net._sample_seed, db=db.tolist(), sc=sc.tolist())))


def _run_child(args):
    code = ("import sys; sys.path[:0] = %r; import test_roidb_cpu as t; t._resume_child(*%r)"
            % ([os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tf-faster-rcnn_amd"),
                os.path.join(ROOT, "tf-faster-rcnn_amd", "lib")], args))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESUMED ")][-1][len("RESUMED "):])


def test_snapshot_mid_epoch_resumes_the_same_sequence_in_a_fresh_process(fixture, data_dir, tmp_path):
    from roi_data_layer.layer import RoIDataLayer
    gp = ggr.case_prefix(True, False)
    want_db, want_sc = fixture[gp + "db_inds"].tolist(), fixture[gp + "scale_inds"].tolist()
    done = 7                                                              # mid-epoch: 12 entries, a permutation serves 11
    with ggr.repo_cfg(data_dir):
        imdb, _, filtered = ggr.repo_roidb()
        np.random.seed(ggr.SEED)
        layer = RoIDataLayer(filtered, imdb.num_classes)
        draw(layer, done)
        sw = _solver(layer)
        sfile, nfile = sw.snapshot(done, str(tmp_path))
        draw(layer, 3)                                                    # the writer goes on; the files do not follow
    with open(nfile, "rb") as f:
        meta = pickle.load(f)
    assert meta["iter"] == done and meta["data_layer"]["cur"] == done and len(meta["data_layer"]["perm"]) == 12 and "np_random_state" in meta
    got = _run_child((data_dir, sfile, nfile, len(want_db) - done, 1, 0))
    assert got["iter"] == done and got["seed"] == 10
    assert got["db"] == want_db[done:] and got["sc"] == want_sc[done:]     # across two reshuffles
    # data parallel: every rank restores the one snapshot and goes on with ITS share of the same stream -- 7 minibatches are drawn, so
    # rank 1 of 2 owns the next one (7 % 2 == 1) and every second one after it, rank 0 of 2 starts one later
    got1 = _run_child((data_dir, sfile, nfile, 5, 2, 1))
    assert got1["db"] == want_db[done::2][:5] and got1["sc"] == want_sc[done::2][:5]
    got0 = _run_child((data_dir, sfile, nfile, 5, 2, 0))
    assert got0["db"] == want_db[done + 1::2][:5] and got0["sc"] == want_sc[done + 1::2][:5]


def test_old_format_snapshot_still_restores(data_dir, tmp_path):
    from roi_data_layer.layer import RoIDataLayer
    with ggr.repo_cfg(data_dir):
        imdb, _, filtered = ggr.repo_roidb()
        np.random.seed(ggr.SEED)
        layer = RoIDataLayer(filtered, imdb.num_classes)
        sw = _solver(layer)
        sfile, nfile = sw.snapshot(4, str(tmp_path))
        with open(nfile, "wb") as f:
            pickle.dump({"iter": 4, "sample_seed": 8}, f, pickle.HIGHEST_PROTOCOL)       # what snapshots held before the data layer existed
        draw(layer, 2)
        cur, perm, state = layer._cur, layer._perm.copy(), np.random.get_state()
        assert sw.restore(sfile, nfile) == 4 and sw.net._sample_seed == 8
        assert layer._cur == cur and np.array_equal(layer._perm, perm)                     # untouched, like the random stream
        assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state()))
        # ... and a synthetic data layer (a generator: no cursor) snapshots / restores as before
        from model.train_val import synthetic_data_layer
        sw2 = _solver(synthetic_data_layer(21))
        s2, n2 = sw2.snapshot(6, str(tmp_path / "syn"))
        with open(n2, "rb") as f:
            assert sorted(pickle.load(f)) == ["iter", "sample_seed"]
        assert sw2.restore(s2, n2) == 6


def test_combined_roidb_joins_names(data_dir, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tf-faster-rcnn_amd", "tools"))
    import importlib
    tool = importlib.import_module("trainval_net")
    with ggr.repo_cfg(data_dir):
        imdb, roidb = tool.combined_roidb("voc_2007_trainval+voc_2007_trainval")
    assert imdb.name == "voc_2007_trainval+voc_2007_trainval" and imdb.num_classes == 21 and len(roidb) == 28
    out = capsys.readouterr().out
    assert "Loaded dataset `voc_2007_trainval` for training" in out and "Set proposal method: gt" in out


@pytest.mark.skipif(not os.path.isdir("/root/reference/lib/roi_data_layer"), reason="reference tree only exists in the build container")
def test_fixture_matches_live_reference():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fixtures", "gen_golden_roidb.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and "bit-exact" in r.stdout, r.stdout + r.stderr
