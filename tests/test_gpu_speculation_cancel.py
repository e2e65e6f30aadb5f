"""GPU: a speculative KL-basis decomposition that is cancelled leaves promptly, writes nothing, and leaves its work area fit for
the next one (k_posterior_eigen_rr: the cancel word is looked at before the start and on a fixed schedule of rounds).

tools/eigen_cancel_check drives the kernel alone; the chain test runs the lone-chain step with speculation adaptive, always and
never: the three chains must be the same chain, and no device-side wait may have timed out on the way."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CHECK = os.path.join(ROOT, "tools", "eigen_cancel_check")


@pytest.mark.parametrize("rank", [5, 32, 33, 50, 51, 64])
def test_cancelled_decomposition_leaves_and_writes_nothing(rank):
    """Ranks: odd and even, one replay workgroup (<= 32 rows) and two, a nearly empty second one (33).  Per rank (see the tool):
    cancelled before the start with `ready` null / raised / raised later — the launch ends, V, Vt, S keep their sentinel bytes,
    the pinned status is not "done"; cancelled 0, 5, …, 100 µs after its input arrived — the launch ends, the outputs are untouched
    or bit-equal to the uncancelled reference; after every case an uncancelled decomposition on the same work area is bit-equal
    (V, Vt, S, sweep count) to the one on a fresh, zeroed work area.  The tool stops at the first launch that does not end in 2 s."""
    assert os.path.exists(CHECK), "build tools/eigen_cancel_check (python -c 'import __graft_entry__ as g; g.build()')"
    p = subprocess.run([CHECK, str(rank)], capture_output=True, text=True, timeout=60)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "rank %d:" % rank in p.stdout and "eigen_cancel_check: ok" in p.stdout


_CHAIN_SCRIPT = r"""
import json, sys, numpy as np
sys.path.insert(0, {root!r})
import __graft_entry__ as graft
pkg = graft.load_package()
model, target = pkg.data.load_femur_model_and_target(50)
setup = pkg.femur_icp_proposal_registration(model, target, fused=2)
ctx = pkg.IcpContext(model, target, device=0)
chain = pkg.SamplingRegistration(ctx, setup, pkg.initial_parameters(model), 1024)
np.save({out!r}, chain.run(400))
json.dump(pkg._native.runtime_stats(), open({stats!r}, "w"))
chain.close(); ctx.close()
"""


@pytest.fixture(scope="module")
def femur50_chains(tmp_path_factory):
    """The bundled femur-50 model and its own target, 400 steps of the lone-chain step: speculation adaptive (default), always
    (ICP_SPECULATION=1) and never (ICP_NO_SPECULATION=1), a child process each -> {tag: (records, runtime stats)}.  Rejected
    steps cancel their decomposition — about three steps in five here — and the next decomposition follows on the same stream
    and work area."""
    tmp = tmp_path_factory.mktemp("speculation_cancel")
    runs = {}
    for tag, env in (("default", {}), ("always", {"ICP_SPECULATION": "1"}), ("never", {"ICP_NO_SPECULATION": "1"})):
        out, stats = str(tmp / (tag + ".npy")), str(tmp / (tag + ".json"))
        base = {k: v for k, v in os.environ.items() if k not in ("ICP_SPECULATION", "ICP_NO_SPECULATION")}
        subprocess.run([sys.executable, "-c", _CHAIN_SCRIPT.format(root=ROOT, out=out, stats=stats)], check=True, env={**base, **env}, timeout=120)
        runs[tag] = (np.load(out), json.load(open(stats)))
        print(tag, "accepted", int(runs[tag][0][:, 1].sum()), runs[tag][1])
    return runs


def test_chain_with_speculation_always_is_the_adaptive_chain(femur50_chains):
    """More than 50 of the 400 steps are accepted, the records with speculation always and adaptive are equal bit for bit, and in
    none of the three runs has a device-side wait timed out or a speculative decomposition given up."""
    for tag, (rec, st) in femur50_chains.items():
        assert st["wait_timeouts"] == 0 and st["speculation_giveups"] == 0, (tag, st)
        assert rec.shape[0] == 400 and rec[:, 1].sum() > 50, tag
    assert np.array_equal(femur50_chains["default"][0], femur50_chains["always"][0]), "speculation always: the chain differs"


def test_chain_without_speculation_is_the_same_chain(femur50_chains):
    """The records without speculation equal the default's bit for bit.

    Every 128th decomposition of a proposal starts cold, and with the count advancing per LAUNCHED decomposition alone the cold
    starts fell on other steps without speculation than with it (same decisions, states to 1.9e-9, 95 of 400 records different
    in their last bits from step 305 on).  A step whose speculation is switched off now keeps the place in the count that its
    launch would have had (icp_proposal::plan_eigen)."""
    a, b = femur50_chains["default"][0], femur50_chains["never"][0]
    differing = np.nonzero(np.abs(a - b).max(axis=1))[0]
    print("decisions equal:", np.array_equal(a[:, 1:3], b[:, 1:3]), "max abs difference:", np.abs(a - b).max(), "records differing:", len(differing),
          "first:", differing[:1])
    assert np.array_equal(a, b), "speculation never: the chain differs"
