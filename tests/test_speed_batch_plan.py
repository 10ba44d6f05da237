"""awm_speed_batch_plan (pure host): which clips of a batched speed search share a sub-group, and what a sub-group's first pass asks
for.  The bytes are restated here from the geometry of the pass (reference wmspeed.cc:461-492, 204-268): 57 centres, per centre the
half-rate copy of the clip and 510 columns of { umag, dmag } per STFT row, both at the stride of the sub-group's largest entry."""
import audiowmark_amd as awm

RATE = 44100


def first_pass_strides(n_frames, channels=2, patient=False):
    seconds, step, n_steps, n_center_steps = (50, 1.00035, 11, 28) if patient else (25, 1.0007, 5, 28)
    clip = min(int(seconds * 1.3 * RATE), n_frames)
    max_out = max_rows = 0
    for c in range(-n_center_steps, n_center_steps + 1):
        speed = step ** (c * (2 * n_steps + 1))
        n_in = min(clip * channels, channels * round(RATE * (seconds / speed))) // channels
        n_out = round(n_in * (speed / 2))
        max_out = max(max_out, n_out)
        max_rows = max(max_rows, (n_out - 512 - 1) // 128 + 1 if n_out > 512 else 0)   # frames of 512 at hop 128, pos + 512 < n_out
    return (max_out * channels + 3) // 4 * 4, (max_rows + 15) // 16 * 16


def group_bytes(frames, channels=2, patient=False):
    strides = [first_pass_strides(n, channels, patient) for n in frames]
    sub, ld = max(s for s, _ in strides), max(l for _, l in strides)
    return len(frames) * 57 * (sub * 4 + 510 * ld * 8)


def test_bytes_of_a_sub_group_are_those_of_its_largest_entry():
    for patient in (False, True):
        for channels in (1, 2, 3):
            for frames in ([30 * RATE], [20 * RATE, 30 * RATE + 7, int(1.2 * RATE)], [int(0.3 * RATE)] * 3):
                groups, nbytes = awm.speed_batch_plan(frames, channels, RATE, patient, budget_bytes=1 << 50)
                assert groups == [0] * len(frames)
                assert nbytes == [group_bytes(frames, channels, patient)], (patient, channels, frames)
    # the figure of DESIGN.md section 10.4: about 1.25 GB for a 30 s stereo clip
    assert 1.2e9 < awm.speed_batch_plan([30 * RATE], budget_bytes=1 << 50)[1][0] < 1.3e9


def test_sub_groups_keep_the_order_and_the_budget():
    long_, short = 30 * RATE, 2 * RATE
    one = group_bytes([long_])
    frames = [long_, long_, short, 100, long_, 0, short, short, long_, long_, long_]
    for budget in (1, one, 2 * one, 3 * one + 5, 1 << 50):
        groups, nbytes = awm.speed_batch_plan(frames, budget_bytes=budget)
        assert [g for g, n in zip(groups, frames) if n < 0.25 * RATE] == [-1, -1]          # under 0.25 s: no search
        part = [(g, n) for g, n in zip(groups, frames) if g >= 0]
        ids = [g for g, _ in part]
        assert ids == sorted(ids) and set(ids) == set(range(len(nbytes)))                   # in call order, numbered from 0
        for gid, b in enumerate(nbytes):
            members = [n for g, n in part if g == gid]
            assert b == group_bytes(members)
            assert b <= budget or len(members) == 1                                         # one clip at least, whatever it costs
        # greedy: a sub-group is closed only by a clip with which it would pass the budget
        for gid in range(len(nbytes) - 1):
            members = [n for g, n in part if g == gid]
            nxt = [n for g, n in part if g == gid + 1][0]
            assert group_bytes(members + [nxt]) > budget
    assert awm.speed_batch_plan(frames, budget_bytes=1)[0] == [0, 1, 2, -1, 3, -1, 4, 5, 6, 7, 8]
    assert awm.speed_batch_plan(frames, budget_bytes=2 * one)[0] == [0, 0, 1, -1, 1, -1, 2, 2, 3, 3, 4]
    assert awm.speed_batch_plan([], budget_bytes=1) == ([], [])


def test_budget_setter_and_default():
    frames = [30 * RATE] * 40
    default = awm.speed_batch_plan(frames)[0]
    try:
        awm.set_speed_batch_bytes(1)
        assert awm.speed_batch_plan(frames)[0] == list(range(40))
        assert awm.speed_batch_plan(frames, budget_bytes=1 << 50)[0] == [0] * 40             # an explicit budget wins
        awm.set_speed_batch_bytes(0)                                                        # 0 restores the default
        assert awm.speed_batch_plan(frames)[0] == default
    finally:
        awm.set_speed_batch_bytes(0)
    assert 1 < default.count(0) < 40 and default[-1] > 0                                    # the default holds several clips, not all
