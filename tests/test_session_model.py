"""The session generator and the state model (tests/session_model.py) held to their claims, on the CPU oracle alone: scripts are
deterministic, the default seeds cover every (operation x rest depth) cell, every pairing, every reader and entry point, and no frame,
operation, delivery or ray batch of theirs is vacuous.  tests/test_gpu_sessions.py plays the same scripts on the renderer."""
import numpy as np
import pytest

import session_model as sm
from zeldaengine_amd import abi

SEEDS = range(sm.DEFAULT_SEEDS)


@pytest.fixture(scope="module")
def scripts():
    return {s: sm.script(s) for s in SEEDS}


def _walk(steps):
    """-> per step (class of the frame before its gap or None, class of its own frame), by the model's own counting"""
    rest, out = sm.Rest(), []
    for s in steps:
        before = rest.last_class
        rest.gap([k for k, _ in s["ops"]], s["advance"])
        rest.frame()
        out.append((before, rest.last_class))
    return out


def test_scripts_are_deterministic(scripts):
    for s in SEEDS:
        again = sm.script(s)
        assert repr(again) == repr(scripts[s]), "seed %d" % s
        assert 24 <= len(again) <= 40, (s, len(again))
        assert eval(repr(again)) == again                     # plain values: a printed script can be pasted back


def test_every_operation_falls_at_every_rest_depth(scripts):
    seen = set()
    for s in SEEDS:
        for step, (before, _) in zip(scripts[s], _walk(scripts[s])):
            seen |= {(k, before) for k, _ in step["ops"] if before is not None}
    missing = [(k, d) for k in sm.OP_KINDS for d in range(4) if (k, d) not in seen]
    assert not missing, missing


def test_every_operation_shares_a_gap_with_another_family(scripts):
    seen = set()
    for s in SEEDS:
        for step in scripts[s]:
            fams = {sm.FAMILY[k] for k, _ in step["ops"]}
            assert len(step["ops"]) <= 3
            seen |= {k for k, _ in step["ops"] if fams - {sm.FAMILY[k]}}
    assert not set(sm.OP_KINDS) - seen, sorted(set(sm.OP_KINDS) - seen)


def test_every_reader_follows_every_rest_depth_and_every_entry_point_occurs(scripts):
    seen, entries = set(), set()
    for s in SEEDS:
        for step, (_, own) in zip(scripts[s], _walk(scripts[s])):
            entries.add(step["entry"])
            seen |= {(k, own) for k, _ in step["readers"]}
            seen.add(("frame" if step["sync"] else "copy_frame_async", own))
    missing = [(k, d) for k in sm.READER_KINDS for d in range(4) if (k, d) not in seen]
    assert not missing, missing
    assert entries == set(sm.ENTRIES)


def test_a_quarter_of_the_seeds_hold_an_unsynchronised_stretch_with_an_operation_inside(scripts):
    n = 0
    for s in SEEDS:
        runs, cur = [], []
        for step in scripts[s]:
            if not step["sync"]:
                cur.append(step)
            elif cur:
                runs.append(cur); cur = []
        if cur:
            runs.append(cur)
        for r in runs:
            assert 4 <= len(r) <= 12, (s, len(r))
            assert all(k in sm.DEVICE_READERS for st in r for k, _ in st["readers"])
        n += any(any(st["ops"] for st in r[1:]) and any(st["readers"] for st in r) for r in runs)
    assert 4 * n >= len(SEEDS), n


class _NotVacuous(sm.Hooks):
    """Plays a seed on the oracle alone and holds every frame, operation, delivery and ray batch to moving what it is there to move."""

    def __init__(self, seed, engine):
        self.seed, self.engine, self.prev = seed, engine, None
        self.moved = True                                     # some frame since the last delivery of changes differs from its predecessor
        self.deliveries = {"read_frame_delta": [0, 0, 0], "read_frame_delta_packed": [0, 0, 0]}      # full, partial, empty

    def frame(self, i, step, m, rest, o):
        what = "seed %d frame %d" % (self.seed, i)
        assert 4 * o.covered_pixels() > m.W * m.H, what
        now = {"shadow": o.shadowmap().view(np.uint32), "gbuffer": [o.gbuffer(t).view(np.uint8) for t in range(6)], "color": o.color()}
        if self.prev is None or self.prev["color"].shape != now["color"].shape or not np.array_equal(self.prev["color"], now["color"]):
            self.moved = True
        for kind, _ in step["ops"]:
            target = sm.MOVES[kind]
            if target is None or self.prev is None or self.prev["color"].shape != now["color"].shape:
                continue
            if target == "color" and kind != "set_debug_view" and (m.view != 0 or (kind == "set_background" and m.sky)):
                continue                                      # (a debug view shows a GBuffer value; a skydome covers the background)
            if target == "gbuffer":
                moved = any(not np.array_equal(a, b) for a, b in zip(self.prev["gbuffer"], now["gbuffer"]))
            else:
                moved = not np.array_equal(self.prev[target], now[target])
            assert moved, "%s: %s did not move the %s" % (what, kind, target)
        self.prev = now

    def reader(self, i, step, reader, m, o):
        what = "seed %d frame %d %s" % (self.seed, i, reader[0])
        kind = reader[0]
        color = o.color()
        if kind in ("raycast", "raycast_async"):
            want = sm.expect(reader, m, o, self.engine, m.free_rays(reader[1]))
            hit = want["flags"] & abi.RAY_HIT_FLAG != 0
            assert hit.any() and not hit.all(), what
        elif kind in ("read_frame_delta", "read_frame_delta_packed"):
            # a delivery lists tiles - it differs from the undelivered frame - unless every frame since the last delivery stood as
            # its predecessor did (the rest the generator put there: a delivery at rest lists nothing, and must)
            before = None if m.delta_full else m.client.copy()
            tiles, pixels, full, f = sm.expect(reader, m, o)
            total = fdr_total(f)
            assert full == (before is None) and (len(tiles) == total) >= full, what
            if not full:
                assert (len(tiles) > 0) == self.moved, "%s: %d tiles listed, the frame %s since the last delivery" % (what, len(tiles), "moved" if self.moved else "stood")
                assert (len(tiles) > 0) == (not np.array_equal(before, f)), what
            self.deliveries[kind][0 if full else 1 if 0 < len(tiles) < total else 2 if len(tiles) == 0 else 0] += 1
            self.moved = False
        elif kind in ("color_highlighted", "read_color_overlaid"):
            want = sm.expect(reader, m, o)
            plain = color if sm.reader_scale(reader) == 1 else sm.fsr.downscale(color, sm.reader_scale(reader))
            assert not np.array_equal(want, plain), what
        elif kind in ("color_scaled", "copy_frame_scaled_async"):
            assert sm.reader_scale(reader) >= 2, what         # (another extent: a scaled delivery differs from the frame by construction)
        elif kind == "read_ids":
            pl = sm.expect(reader, m, o)
            assert len(np.unique(pl[..., 0])) >= 3, what
        elif kind in ("instance_coverage", "instance_coverage_async"):
            cov = sm.expect(reader, m, o)
            assert int(cov.sum()) == o.covered_pixels() and (cov > 0).sum() >= 3, what
        elif kind == "pick":
            hits, total = sm.expect(reader, m, o)
            assert total >= 1 and len(hits) == total, what
        else:
            raise ValueError(kind)


def fdr_total(f):
    nx, ny = sm.fdr.tile_grid(f.shape[1], f.shape[0])
    return nx * ny


@pytest.fixture(scope="module")
def played(oracle_lib, scripts):
    """every default seed played once on the oracle: seed -> (the hooks with their counts, the failure or None)"""
    from zeldaengine_amd import engine
    out = {}
    for seed in SEEDS:
        h, err = _NotVacuous(seed, engine), None
        try:
            sm.run(scripts[seed], seed=seed, oracle_lib=oracle_lib, hooks=h)
        except AssertionError as e:
            err = e
        out[seed] = (h, err)
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_no_frame_operation_delivery_or_ray_batch_is_vacuous(played, seed):
    if played[seed][1] is not None:
        raise played[seed][1]


def test_deliveries_of_changes_come_full_partial_and_at_rest(played):
    """over the default seeds both forms deliver a whole frame, a part of one (0 < tiles < total) and, at rest, nothing; deliveries at
    rest are the smaller part"""
    for kind in ("read_frame_delta", "read_frame_delta_packed"):
        full, partial, empty = (sum(h.deliveries[kind][j] for h, _ in played.values()) for j in range(3))
        print(kind, "full", full, "partial", partial, "empty", empty)
        assert full > 0 and partial > 0 and empty > 0 and 2 * empty < full + partial + empty, (kind, full, partial, empty)


def test_every_flavour_and_starting_state_occurs():
    starts = [sm.start(s) for s in SEEDS]
    assert {(st["flags"], st["sky"]) for st in starts} == {(0, False), (abi.FLAG_SERIAL_PASSES, False), (abi.FLAG_NO_LIST_REUSE, False), (0, True)}
    for key in ("extent", "SD", "n_point", "capture", "big_image", "stretch"):
        assert len({st[key] for st in starts}) == 2, key
    assert 2 * sum(st["flags"] == 0 and not st["sky"] for st in starts) >= len(starts) // 2      # the keep assertions need default contexts
