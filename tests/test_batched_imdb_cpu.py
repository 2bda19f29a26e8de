"""CPU: model.test.plan_batches -- the order in which test_net_imdb walks an imdb under cfg.HIP.TEST_BATCH_IMAGES: same-size images together,
full batches first, a remainder padded or run one by one, every image exactly once -- and the switch's default."""
import pytest

A, B, C = (375, 500), (500, 375), (480, 640)


def check_plan(sizes, batch):
    """the properties every plan has; returns it"""
    from model.test import plan_batches
    plan = plan_batches(sizes, batch)
    seen = [i for idx, _ in plan for i in idx]
    assert sorted(seen) == list(range(len(sizes))) and len(seen) == len(sizes)          # every index exactly once among the non-pad slots
    for idx, pad in plan:
        assert len(idx) >= 1 and pad >= 0
        assert len({tuple(sizes[i]) for i in idx}) == 1                                  # one size per entry
        assert list(idx) == sorted(idx)
        assert len(idx) + pad in (1, batch)                                              # no graph of an odd batch size
        assert pad == 0 or (len(idx) + pad == batch and 2 * len(idx) >= batch)
    return plan


def test_batch_one_is_the_identity_order():
    sizes = [A, B, A, C, B, A]
    assert check_plan(sizes, 1) == [([i], 0) for i in range(6)]
    assert check_plan([], 1) == [] and check_plan([], 4) == []


def test_full_batches_come_first_then_the_remainder_rule():
    # r = 3 of batch 4 (2r >= batch): padded by one;  r = 2 of 4 (2r == batch): padded by two;  r = 1 of 4: a single
    assert check_plan([A] * 11, 4) == [([0, 1, 2, 3], 0), ([4, 5, 6, 7], 0), ([8, 9, 10], 1)]
    assert check_plan([A] * 6, 4) == [([0, 1, 2, 3], 0), ([4, 5], 2)]
    assert check_plan([A] * 5, 4) == [([0, 1, 2, 3], 0), ([4], 0)]
    assert check_plan([A] * 4, 4) == [([0, 1, 2, 3], 0)]
    # batch 8: r = 3 -> three singles, r = 4 -> padded by four, r = 7 -> padded by one
    assert check_plan([A] * 11, 8) == [(list(range(8)), 0), ([8], 0), ([9], 0), ([10], 0)]
    assert check_plan([A] * 12, 8) == [(list(range(8)), 0), ([8, 9, 10, 11], 4)]
    assert check_plan([A] * 7, 8) == [(list(range(7)), 1)]
    # an odd batch: r = 1 of 3 is below half (2 < 3), r = 2 is above
    assert check_plan([A] * 4, 3) == [([0, 1, 2], 0), ([3], 0)]
    assert check_plan([A] * 5, 3) == [([0, 1, 2], 0), ([3, 4], 1)]
    assert check_plan([A] * 1, 2) == [([0], 1)]


def test_interleaved_groups_come_out_contiguous_in_order_of_first_appearance():
    sizes = [A, B, A, B, A, B, A, B, A, C]
    plan = check_plan(sizes, 2)
    assert plan == [([0, 2], 0), ([4, 6], 0), ([8], 1), ([1, 3], 0), ([5, 7], 0), ([9], 1)]
    # each shape's entries are adjacent: its graphs are used in one run, not revisited
    shapes = [sizes[idx[0]] for idx, _ in plan]
    assert [s for k, s in enumerate(shapes) if k == 0 or shapes[k - 1] != s] == [A, B, C]


def test_the_layout_of_the_gpu_test():
    sizes = [(120, 160)] * 3 + [(160, 120)] + [(120, 160)] * 2 + [(160, 120)] * 2 + [(96, 160)] + [(120, 160)] * 1 + [(160, 120)]
    assert check_plan(sizes, 4) == [([0, 1, 2, 4], 0), ([5, 9], 2), ([3, 6, 7, 10], 0), ([8], 0)]


@pytest.mark.parametrize("batch", [2, 3, 4, 8])
def test_properties_on_a_mixed_list(batch):
    sizes = [(A, B, C, A, A, B)[(i * 7 + i // 5) % 6] for i in range(41)] + [(7, 9)]
    check_plan(sizes, batch)
    check_plan([list(s) for s in sizes], batch)                                          # lists as well as tuples


def test_the_switch_is_off_by_default():
    from model.config import cfg
    assert cfg.HIP.TEST_BATCH_IMAGES == 1


def test_the_batched_loop_refuses_an_unlimited_record_before_any_work():
    """max_per_image <= 0 is the one-by-one loop's form (test_net_imdb keeps that loop for it); asked of the batched functions directly it
    is an error raised before a file is opened or anything is staged"""
    from model.test import detect_bgr_batch, detect_paths_batched
    for bad in (0, -1):
        with pytest.raises(ValueError, match="max_per_image"):
            detect_paths_batched(None, None, ["/no/such/file.jpg"], 4, max_per_image=bad)
        with pytest.raises(ValueError, match="max_per_image"):
            detect_bgr_batch(None, None, None, max_per_image=bad)
