"""The plan layer of the convolution GEMMs (csrc/conv_plan.h) answers what the code before it answered.

tests/golden/conv_plans.npz was recorded from the commit before the plan layer existed (tests/golden/make_conv_plans.py
says how): per descriptor and setting the forward plan, the weight-gradient plan for dense and for padded gy rows, the
three legacy queries, the grouped plans, and the kernel labels the Python binding derived at that commit.  The same
recording code runs here against the built library — pure host code, no GPU — and every column must be equal."""
import json
import os

import numpy as np
import pytest

from tests.golden import make_conv_plans as G

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans.npz")


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(FIXTURE))


@pytest.fixture(scope="module")
def current(recorded):
    from da_detect_amd import _lib

    rows = [tuple(int(v) for v in r) for r in recorded["desc"]]
    return G.record(_lib.load(), rows, names_from_plan=True)


def test_fixture_covers_the_issue_grid_and_every_kernel_family(recorded):
    assert json.loads(str(recorded["settings"])) == json.loads(json.dumps(G.SETTINGS))
    assert [tuple(int(v) for v in r) for r in recorded["desc"]] == G.descriptors()
    ok = recorded["fwd_rc"] == 0
    for f, name in enumerate(G.FWD_FAMILIES):
        assert (recorded["fwd_family"][ok] == f).any(), "no descriptor of the fixture reaches forward family %s" % name
    for f, name in enumerate(G.WGRAD_FAMILIES):
        assert (recorded["wgrad_family"] == f).any(), "no descriptor of the fixture reaches weight-gradient family %s" % name
    assert set(recorded["group_kind"].tolist()) >= {0, 128, 256}
    assert os.path.getsize(FIXTURE) < 256 * 1024


def test_plans_equal_the_recorded_ones_row_by_row(recorded, current):
    ndesc = len(recorded["desc"])
    settings = json.loads(str(recorded["settings"]))
    failures = []

    def where(i, per_setting):
        s, k = divmod(int(i), per_setting)
        return "setting %s" % (settings[s],), s, k

    for key in sorted(recorded):
        if key in ("desc", "settings", "names") or key.endswith("_name"):
            continue
        a, b = recorded[key], current[key]
        assert a.shape == b.shape, key
        bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
        for i in bad[:3]:
            if key.startswith("group_"):
                failures.append("%s: %s group %d: recorded %s, now %s" % (key, where(i, len(G.GROUPS))[0], i % len(G.GROUPS),
                                                                           a[i], b[i]))
            elif key.startswith("wgradld_"):
                failures.append("%s: padded-row entry %d: recorded %s, now %s" % (key, i, a[i], b[i]))
            else:
                text, _, k = where(i, ndesc)
                failures.append("%s: %s %s: recorded %s, now %s" % (key, text, dict(zip(G.DESC_FIELDS, recorded["desc"][k])),
                                                                    a[i], b[i]))
    # kernel labels: what the plan entry points say now against what the binding derived from the legacy queries
    for key in ("fwd_name", "wgrad_name", "wgradld_name"):
        a, b = recorded["names"][recorded[key]], current["names"][current[key]]
        for i in np.nonzero(a != b)[0][:3]:
            failures.append("%s: row %d: recorded %r, now %r" % (key, i, a[i], b[i]))
    assert not failures, "\n".join(failures)
