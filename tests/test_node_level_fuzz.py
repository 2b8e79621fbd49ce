"""Randomised sessions of the node-level interface (lbft_batch_manual_begin, lbft_node_*, lbft_node_calls) against the oracle.

A seeded driver plays the network by hand over one instance: it mostly follows the NodeUpdateActions the nodes return, so sessions
make progress, and otherwise perturbs clocks (large jumps that force timeouts and TCs), delivery (late, twice, to a subset, never,
stale after rounds moved on), the record exchange (late or duplicated responses) and the lifetime of handles, and takes save_node
images at random points.  Every call runs on the implementation under test and on the oracle:
  * after every call: the actions, should_sync and the view of every node the call touched equal the oracle's; handles are checked
    for validity (the oracle numbers its messages differently) -- and on the device, equal to the host build's for the same call;
  * at the end: every node's view, commit count, committed history, last committed State, epoch, record hashes and save_node image;
    the instance's fault word is zero.
A fault is accepted only as a capacity limit of the harness's snapshot pool: the same session with room must then equal the oracle.

CPU tier: the host build of the kernel logic (oracle_ctypes.HostSession, node_op_body of csrc/lbft_node_ops.h -- the code the device
kernels run).  GPU tier (-m gpu): the same sessions through NodeHandle (one launch per call) and through BatchSimulator.node_calls
(many instances, each with its own session, one call per instance and launch).
"""
import random

import numpy as np
import pytest

LBFT_MAX_CLOCK = 0x7FFFFFFD
UPDATE, CREATE_NOTE, HANDLE_NOTE, RELEASE, CREATE_REQ, HANDLE_REQ, HANDLE_RESP = range(7)  # LBFT_CALL_*
NODES = (1, 2, 3, 4, 5, 7, 16, 31, 32, 33, 40, 64, 65, 100, 128)


# ---------------------------------------------------------------------------------------------------------------------------------
# Session configurations
# ---------------------------------------------------------------------------------------------------------------------------------
def draw_spec(seed, n=None, quirks=None, exchange_big=False):
    """One session's configuration: network, NodeConfig, epochs, quirks, equivocation, clocks and how long it runs."""
    r = random.Random(seed * 7919 + 17)
    n = n if n is not None else r.choice(NODES)
    quirks = quirks if quirks is not None else r.randrange(4)
    if exchange_big:
        quirks |= 1
    weighted = n > 1 and r.random() < 0.4
    rights = [r.randint(1, 5) for _ in range(n)] if weighted else None
    epochs = r.random() < 0.45
    spec = dict(
        seed=seed, n=n, quirks=quirks, voting_rights=rights,
        rights_rotation=r.randrange(1, n) if weighted and epochs and n > 1 and r.random() < 0.6 else 0,
        commands_per_epoch=r.choice((2, 3, 5, 8)) if epochs else 30000,
        keep_stores=epochs,
        delta=r.choice((3, 5, 10, 20, 40)), gamma=r.choice((1.0, 1.5, 2.0)), lambda_=r.choice((0.25, 0.5, 0.75)),
        target_commit_interval=r.choice((1, 10, 100, 100000)),
        equivocate_every=r.choice((0, 0, 0, 2, 3)) if n >= 4 else 0,
        # (the archive of retired stores of a large network must fit the 2^24 rows of an instance: lbft_batch_manual_begin)
        max_clock=r.choice((1000, 5000) if epochs and n > 32 else (1000, 5000, 20000)),
        past_max_clock=r.random() < 0.2,  # the session's clocks run past the session's max_clock, up to LBFT_MAX_CLOCK
    )
    # calls per session: large networks need several hundred per round
    spec["steps"] = int(r.choice((300, 600, 1000)) * (1 + n / 12))
    spec["calm"] = exchange_big  # no clock jumps: the large exchange sessions are to reach rounds led by authors >= 64
    return spec


def oracle_config(oracle, spec):
    return oracle.make_config(num_nodes=spec["n"], math_mode=1, commands_per_epoch=spec["commands_per_epoch"],
                              target_commit_interval=spec["target_commit_interval"], delta=spec["delta"], gamma=spec["gamma"],
                              lambda_=spec["lambda_"], quirks=spec["quirks"], voting_rights=spec["voting_rights"],
                              equivocate_every=spec["equivocate_every"], rights_rotation=spec["rights_rotation"])


# ---------------------------------------------------------------------------------------------------------------------------------
# The driver: a generator per session that yields calls and receives their (compared) results
# ---------------------------------------------------------------------------------------------------------------------------------
class Msg:
    """A notification / request / response: the model's handle and the oracle's."""
    __slots__ = ("m", "o", "uses", "kind", "sender")

    def __init__(self, m, o, kind, sender):
        self.m, self.o, self.kind, self.sender, self.uses = m, o, kind, sender, 0


def session(spec, stats):
    """Yields (op, node, peer, msg, node_time) and receives the call's result (a dict; "msg" holds the new Msg of a create)."""
    r = random.Random(spec["seed"])
    n, q1 = spec["n"], spec["quirks"] & 1
    clock = [0] * n
    T = 0
    due = [0] * n               # the next_scheduled_update each node asked for
    inbox = []                  # [ready_at, kind, receiver, msg]
    parked = []                 # messages whose last use is over but which are held before the release
    delivered = set()           # (receiver, id(msg)) -- duplicates are counted

    def now(k):
        clock[k] = max(clock[k], T - r.randrange(3))
        return clock[k]

    def post(kind, receiver, msg, delay):
        msg.uses += 1
        inbox.append([T + delay, kind, receiver, msg])

    def done_with(msg):
        msg.uses -= 1
        if msg.uses == 0:
            parked.append(msg)

    # time moves about once per call of every node, so that cooperative rounds can finish before their timers; jumps force timeouts
    tick = min(0.5, 0.6 / n)
    jump = 0.0 if spec["calm"] else r.choice((0.0, 0.002, 0.01)) * tick
    step = 0
    while step < spec["steps"]:
        step += 1
        # clocks: mostly small steps, sometimes a jump that makes the pacemakers time out
        x = r.random()
        if x < jump:
            T += r.randint(20, 200) * spec["delta"]
        elif x < tick:
            T += r.randint(1, 3)
        if spec["past_max_clock"] and step == spec["steps"] // 2:
            T = max(T, r.choice((spec["max_clock"], spec["max_clock"] + 1, LBFT_MAX_CLOCK - 10 ** 6, LBFT_MAX_CLOCK // 2)))
        T = min(T, LBFT_MAX_CLOCK - 10 ** 4)
        # releases of parked handles, some held long
        while parked and (r.random() < 0.6 or len(parked) > 40):
            msg = parked.pop(r.randrange(len(parked)) if r.random() < 0.3 else 0)
            yield (RELEASE, msg.sender, 0, msg, 0)
        ready = [e for e in inbox if e[0] <= T]
        if ready and r.random() < 0.75:
            e = ready[0] if r.random() < 0.8 else r.choice(ready)
            inbox.remove(e)
            _, kind, k, msg = e
            if r.random() < 0.04:  # lost
                done_with(msg)
                continue
            if r.random() < 0.05:  # delivered twice (the second copy arrives later)
                post(kind, k, msg, r.randint(0, 40))
            key = (k, id(msg))
            if key in delivered:
                stats["duplicate"] += 1
            delivered.add(key)
            if kind == "note":
                res = yield (HANDLE_NOTE, k, msg.sender, msg, 0)
                if res["round_moved"]:
                    stats["stale"] += 1
                if res["should_sync"]:
                    stats["should_sync"] += 1
                    # DataSyncNode: ask the sender (quirks bit 0) or, in reference mode, answer oneself
                    req = (yield (CREATE_REQ, k, 0, None, 0))["msg"]
                    if req is not None:
                        if q1:
                            post("req", msg.sender, req, r.randint(0, 6))
                        else:
                            resp = (yield (HANDLE_REQ, k, 0, req, 0))["msg"]
                            yield (HANDLE_RESP, k, k, resp, now(k))
                            parked.extend([req, resp])
                due[k] = min(due[k], T)
            elif kind == "req":
                resp = (yield (HANDLE_REQ, k, 0, msg, 0))["msg"]
                if resp is not None:
                    requester = msg.sender
                    post("resp", requester, resp, r.randint(0, 10) if r.random() < 0.8 else r.randint(20, 200))
                    if r.random() < 0.05:
                        post("resp", requester, resp, r.randint(0, 60))
            else:  # "resp"
                res = yield (HANDLE_RESP, k, msg.sender, msg, now(k))
                if res["changed"]:
                    stats["insert"] += 1
                    if n > 32:
                        stats["exchange_big"] += 1
                due[k] = min(due[k], T)
            done_with(msg)
            continue
        # an update: a node whose timer is due, or any node
        cands = [k for k in range(n) if due[k] <= T]
        k = r.choice(cands) if cands and r.random() < 0.85 else r.randrange(n)
        res = yield (UPDATE, k, 0, None, now(k))
        a = res["actions"]
        due[k] = a["next_scheduled_update"]
        receivers = [j for j in range(n) if j != k] if a["should_broadcast"] else [j for j in a["should_send"] if j != k]
        if any(j >= 64 for j in a["should_send"]):
            stats["send64"] += 1
        if receivers and r.random() < 0.97:
            msg = (yield (CREATE_NOTE, k, 0, None, 0))["msg"]
            if msg is None:
                continue
            if r.random() < 0.1:  # to a subset
                receivers = [j for j in receivers if r.random() < 0.5]
            late = r.random() < 0.05
            for j in receivers:
                post("note", j, msg, r.randint(0, 4) if not late else r.randint(30, 300))
            if not receivers:
                parked.append(msg)
        if a["should_query_all"] and n > 1:
            req = (yield (CREATE_REQ, k, 0, None, 0))["msg"]
            if req is not None:
                if q1:
                    for j in r.sample([j for j in range(n) if j != k], min(n - 1, 3)):
                        post("req", j, req, r.randint(0, 6))
                else:
                    resp = (yield (HANDLE_REQ, k, 0, req, 0))["msg"]
                    yield (HANDLE_RESP, k, k, resp, now(k))
                    parked.extend([req, resp])
        if r.random() < 0.02:
            yield ("save", r.randrange(n), 0, None, 0)
    # drain: every handle still held is released at the end
    for e in inbox:
        e[3].uses = 0
    for msg in {id(e[3]): e[3] for e in inbox}.values():
        yield (RELEASE, msg.sender, 0, msg, 0)
    for msg in parked:
        yield (RELEASE, msg.sender, 0, msg, 0)


def new_stats():
    return dict(calls=0, commits=0, epochs=0, tc=0, should_sync=0, insert=0, send64=0, exchange_big=0, stale=0, duplicate=0)


# ---------------------------------------------------------------------------------------------------------------------------------
# Runner: one call on the model and on the oracle, compared
# ---------------------------------------------------------------------------------------------------------------------------------
class Capacity(Exception):
    """The model's snapshot pool ran out (a harness capacity limit, not a difference)."""


class OracleSide:
    def __init__(self, oracle, spec):
        self.sim = oracle.OracleSim(oracle_config(oracle, spec), spec["seed"])

    def call(self, op, node, peer, msg, t):
        s = self.sim
        if op == UPDATE:
            return {"actions": s.node_update(node, t)}
        if op == CREATE_NOTE:
            return {"handle": s.node_create_notification(node)}
        if op == HANDLE_NOTE:
            return {"should_sync": s.node_handle_notification(node, msg.o)}
        if op == CREATE_REQ:
            return {"handle": s.node_create_request(node)}
        if op == HANDLE_REQ:
            return {"handle": s.node_handle_request(node, msg.o)}
        if op == HANDLE_RESP:
            s.node_handle_response(node, msg.o, t)
        return {}


def model_args(call):
    op, node, peer, msg, t = call
    return (op, node, peer, msg.m if msg is not None else 0, t)


def check_result(call, got, want, q1):
    """Compares one call's model result with the oracle's -> the driver's result (new Msg for creates)."""
    op, node, peer, msg, t = call
    res = {"msg": None, "should_sync": False, "actions": None}
    if got.get("status", 0) != 0:
        raise Capacity(call)
    if op == UPDATE:
        assert got["actions"] == want["actions"], (call, got["actions"], want["actions"])
        res["actions"] = got["actions"]
    elif op == HANDLE_NOTE:
        assert got["should_sync"] == want["should_sync"], call
        res["should_sync"] = got["should_sync"]
    elif op in (CREATE_NOTE, CREATE_REQ, HANDLE_REQ):
        h = got["handle"]
        kind = {CREATE_NOTE: "note", CREATE_REQ: "req", HANDLE_REQ: "resp"}[op]
        res["msg"] = Msg(h, want["handle"], kind, node)
    return res


def touched(call):
    op, node = call[0], call[1]
    return node if op in (UPDATE, HANDLE_NOTE, HANDLE_RESP) else None


def drive_single(model, inst, oracle_side, spec, stats, scap, view_every=1):
    """Runs one session through `model` (call(op, inst, node, peer, handle, t) / view / save_node) call by call."""
    gen = session(spec, stats)
    q1 = spec["quirks"] & 1
    live = {}
    res = None
    views = {}
    while True:
        try:
            call = gen.send(res)
        except StopIteration:
            break
        op, node = call[0], call[1]
        if op == "save":
            img = model.save_node(inst, node)
            if img is not None:
                assert img == oracle_side.sim.save_node(node), ("save_node", call)
                stats["saves"] = stats.get("saves", 0) + 1
            res = None
            continue
        stats["calls"] += 1
        before = views.get(node)
        got = model.call(*(model_args(call)[:1] + (inst,) + model_args(call)[1:]))
        want = oracle_side.call(*call)
        try:
            res = check_result(call, got, want, q1)
        except AssertionError:
            if model.hs.fault(inst)[0]:  # a pool of the harness ran out (F_BLOCK_OVERFLOW, F_SNAP_OVERFLOW, ...)
                raise Capacity(call)
            raise
        if res["msg"] is not None:
            h = res["msg"].m
            if q1 or op == CREATE_NOTE:
                assert h < scap and h not in live, (call, h)
                live[h] = res["msg"]
        if op == RELEASE and (q1 or call[3].kind == "note"):
            live.pop(call[3].m, None)
        k = touched(call)
        res["round_moved"] = res["changed"] = False
        if k is not None and stats["calls"] % view_every == 0:
            v = model.view(inst, k)
            assert v == oracle_side.sim.node_view(k), (call, v)
            if before is not None:
                res["changed"] = v != before
                res["round_moved"] = v["current_round"] > before["current_round"]
            views[k] = v
            stats["tc"] += v["has_timeout_certificate"]
    return live


def compare_end(model_end, oracle_side, spec, stats):
    """End-of-session read-backs of the model (a dict per node) against the oracle."""
    sim = oracle_side.sim
    n = spec["n"]
    for k in range(n):
        e = model_end[k]
        assert e["view"] == sim.node_view(k), k
        hist = sim.committed_history(k)
        assert e["commit_count"] == len(hist), k
        assert (e["history"] == hist).all(), k
        assert e["last_state"] == sim.last_committed_states()[k], k
        assert e["view"]["epoch_id"] == sim.epochs()[k], k
        ref = sim.committed_record_hashes(k)
        got = e["record_hashes"]
        assert len(got) == len(ref), k
        assert (got[:, 0] == ref["block_hash"]).all() and (got[:, 1] == ref["state"]).all() and (got[:, 2] == ref["qc_hash"]).all(), k
        assert ((got[:, 3] & 0xffffffff) == ref["num_votes"]).all(), k
        if e["image"] is not None:
            assert e["image"] == sim.save_node(k), ("save_node", k)
        elif not spec["keep_stores"]:
            assert e["view"]["epoch_id"] > 0, k  # (only a node past epoch 0 lacks an image, and only without keep_stores)
    stats["commits"] += sum(model_end[k]["commit_count"] for k in range(n))
    stats["epochs"] += max(model_end[k]["view"]["epoch_id"] for k in range(n))


def host_end(hs, inst, n):
    out = []
    for k in range(n):
        hist, st = hs.committed_history(inst, k)
        out.append(dict(view=hs.view(inst, k), commit_count=len(hist), history=hist, last_state=st,
                        record_hashes=hs.committed_record_hashes(inst, k, len(hist)), image=hs.save_node(inst, k)))
    return out


def roomy_caps(oracle, spec):
    """Capacities with room: eight times the session's snapshot and block pools."""
    caps = oracle.manual_caps(spec["n"], spec["quirks"], spec["max_clock"], keep_stores=spec["keep_stores"])
    return dict(snapshot_capacity=min(65535, 8 * caps["scap"]), block_capacity=min(65534, 8 * caps["bcap"]))


def run_host_session(oracle, spec, room=None):
    """One session on the host build -> (stats, session); raises Capacity when a pool of the session ran out."""
    caps = oracle.manual_caps(spec["n"], spec["quirks"], spec["max_clock"], keep_stores=spec["keep_stores"], **(room or {}))
    hs = oracle.HostSession(oracle_config(oracle, spec), [spec["seed"]], spec["max_clock"], caps)
    hs.hs = hs
    stats = new_stats()
    ora = OracleSide(oracle, spec)
    drive_single(hs, 0, ora, spec, stats, caps["scap"])
    fault, live, most = hs.fault(0)
    if fault:
        raise Capacity(fault)
    assert live == 0, ("snapshot slots leaked", live)  # every handle was released
    compare_end(host_end(hs, 0, spec["n"]), ora, spec, stats)
    stats["most_slots"] = most
    return stats, hs


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------------------
HOST_SEEDS = list(range(1, 97))
# large networks with the record exchange (peer-answered requests above 32 nodes)
HOST_EXCHANGE_BIG = [(33, 1001), (40, 1002), (65, 1003), (100, 1004), (128, 1005)]
_COVERAGE = {}


def host_session(oracle, spec):
    try:
        return run_host_session(oracle, spec)
    except Capacity:
        # a harness capacity limit: with room the same session must equal the oracle
        stats, hs = run_host_session(oracle, spec, room=roomy_caps(oracle, spec))
        stats["capacity_retries"] = 1
        return stats, hs


@pytest.mark.parametrize("chunk", range(8))
def test_host_sessions_equal_the_oracle(oracle, chunk):
    for seed in HOST_SEEDS[chunk::8]:
        stats, _ = host_session(oracle, draw_spec(seed))
        _COVERAGE[("drawn", seed)] = stats


@pytest.mark.parametrize("n,seed", HOST_EXCHANGE_BIG)
def test_host_sessions_with_record_exchange_on_large_networks(oracle, n, seed):
    spec = draw_spec(seed, n=n, exchange_big=True)
    stats, _ = host_session(oracle, spec)
    _COVERAGE[("exchange", seed)] = stats


def test_host_coverage_of_the_drawn_sessions(oracle):
    """What the sessions above reached (each test module run computes them once; run alone, this test drives them itself)."""
    for seed in HOST_SEEDS:
        if ("drawn", seed) not in _COVERAGE:
            _COVERAGE[("drawn", seed)] = host_session(oracle, draw_spec(seed))[0]
    for n, seed in HOST_EXCHANGE_BIG:
        if ("exchange", seed) not in _COVERAGE:
            _COVERAGE[("exchange", seed)] = host_session(oracle, draw_spec(seed, n=n, exchange_big=True))[0]
    tot = {k: sum(s.get(k, 0) for s in _COVERAGE.values()) for k in list(new_stats()) + ["saves", "capacity_retries"]}
    print("node-level fuzz coverage (%d sessions):" % len(_COVERAGE), tot)
    assert tot["commits"] > 0 and tot["epochs"] > 0, tot
    assert tot["tc"] > 0 and tot["should_sync"] > 0 and tot["insert"] > 0, tot
    assert tot["send64"] > 0 and tot["exchange_big"] > 0, tot
    assert tot["stale"] + tot["duplicate"] > 0, tot
    assert tot["saves"] > 0, tot


def test_host_snapshot_pool_frees_released_slots_and_fails_cleanly_when_full(oracle):
    """A fresh manual session holds no snapshot slot: with a pool of CAP slots a long session that creates far more handles than CAP but
    keeps few live never faults; CAP live handles fill it, the next create fails (-1 slot, F_SNAP_OVERFLOW) and, after releases, the
    session goes on equal to the oracle."""
    spec = dict(draw_spec(5, n=4, quirks=1), equivocate_every=0)
    stats, hs = run_pool_session(oracle, lambda: oracle.HostSession(oracle_config(oracle, spec), [spec["seed"]], spec["max_clock"],
                                                                    oracle.manual_caps(4, 1, spec["max_clock"], POOL_CAP)), spec)
    assert stats["creates"] > 8 * POOL_CAP and stats["full_at"] == POOL_CAP


POOL_CAP = 8


class HostInst:
    """The calls of one instance of a host session, in the shape drive_pool uses (call / view / fault)."""
    def __init__(self, hs, inst=0):
        self.hs, self.inst = hs, inst

    def call(self, op, node, peer, handle, t):
        return self.hs.call(op, self.inst, node, peer, handle, t)

    def view(self, node):
        return self.hs.view(self.inst, node)


def run_pool_session(oracle, make, spec, wrap=HostInst):
    model = wrap(make())
    ora = OracleSide(oracle, spec)
    live0 = model.hs.fault(0)[1] if getattr(model, "hs", None) is not None else 0
    assert live0 == 0  # a fresh manual session holds no slot
    stats = dict(creates=0, full_at=None)
    n, T = spec["n"], 0

    def both(op, node, peer, msg, t):
        got = model.call(op, node, peer, msg.m if msg else 0, t)
        if got.get("status", 0):
            return got, None
        return got, check_result((op, node, peer, msg, t), got, ora.call(op, node, peer, msg, t), 1)

    for rnd in range(200):  # cooperative rounds; every notification released right after its deliveries
        T += 1
        for k in range(n):
            _, res = both(UPDATE, k, 0, None, T)
            if res["actions"]["should_broadcast"] or res["actions"]["should_send"]:
                _, c = both(CREATE_NOTE, k, 0, None, 0)
                stats["creates"] += 1
                rec = [j for j in range(n) if j != k] if res["actions"]["should_broadcast"] else res["actions"]["should_send"]
                for j in rec:
                    both(HANDLE_NOTE, j, k, c["msg"], 0)
                both(RELEASE, k, 0, c["msg"], 0)
        for k in range(n):
            assert model.view(k) == ora.sim.node_view(k), (rnd, k)
    assert ora.sim.node_view(0)["commit_count"] > 5
    held = []
    for i in range(POOL_CAP + 1):  # fill the pool
        got, c = both(CREATE_NOTE, i % n, 0, None, 0)
        if c is None:
            assert got["status"] == -5 and stats["full_at"] is None
            stats["full_at"] = len(held)
            break
        held.append(c["msg"])
    for msg in held:
        both(RELEASE, msg.sender, 0, msg, 0)
    for k in range(n):  # and the session goes on
        T += 1
        _, res = both(UPDATE, k, 0, None, T)
        assert model.view(k) == ora.sim.node_view(k)
    return stats, model


def test_host_node_times_past_max_clock_equal_the_oracle(oracle):
    """Node times at and beyond the session's max_clock, up to LBFT_MAX_CLOCK, on the host build."""
    for n, quirks in ((4, 0), (40, 1)):
        spec = dict(draw_spec(11, n=n, quirks=quirks), max_clock=1000, equivocate_every=0)
        hs = oracle.HostSession(oracle_config(oracle, spec), [11], 1000, oracle.manual_caps(n, quirks, 1000))
        ora = OracleSide(oracle, spec)
        for t in (999, 1000, 1001, 5 * 10 ** 5, LBFT_MAX_CLOCK - 100, LBFT_MAX_CLOCK):
            for k in range(n):
                got = hs.call(UPDATE, 0, k, 0, 0, t)
                assert got["actions"] == ora.call(UPDATE, k, 0, None, t)["actions"], (n, t, k)
                assert hs.view(0, k) == ora.sim.node_view(k), (n, t, k)
        assert hs.fault(0)[0] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------------------
def device_batch(amd, spec, seeds, snapshot_capacity=0, lanes_per_wavefront=0):
    nc = amd.NodeConfig(spec["target_commit_interval"], spec["delta"], spec["gamma"], spec["lambda_"])
    sim = amd.BatchSimulator.new(np.asarray(seeds, dtype=np.uint64), spec["n"], amd.RandomDelay.new(10.0, 4.0), nc,
                                 commands_per_epoch=spec["commands_per_epoch"], voting_rights=spec["voting_rights"],
                                 snapshot_capacity=snapshot_capacity, quirks=spec["quirks"], equivocate_every=spec["equivocate_every"],
                                 rights_rotation=spec["rights_rotation"], keep_retired_stores=spec["keep_stores"],
                                 lanes_per_wavefront=lanes_per_wavefront)
    nodes = sim.manual(spec["max_clock"])
    return sim, nodes


class DeviceSingle:
    """NodeHandle (one launch per call), shadowed by the host build: every result, handles included, must equal the host's."""
    def __init__(self, amd, oracle, spec, snapshot_capacity=0):
        self.amd = amd
        self.sim, nodes = device_batch(amd, spec, [spec["seed"]], snapshot_capacity)
        self.nodes = nodes[0]
        caps = oracle.manual_caps(spec["n"], spec["quirks"], spec["max_clock"], snapshot_capacity, spec["keep_stores"])
        self.host = oracle.HostSession(oracle_config(oracle, spec), [spec["seed"]], spec["max_clock"], caps)
        self.hs = self.host

    def call(self, op, inst, node, peer, handle, t):
        amd, h = self.amd, self.nodes[node]
        r = {"actions": None, "handle": 0, "should_sync": False, "status": 0}
        try:
            if op == UPDATE:
                r["actions"] = h.update_node(t)
            elif op == CREATE_NOTE:
                r["handle"] = h.create_notification()[1]
            elif op == HANDLE_NOTE:
                r["should_sync"] = h.handle_notification((peer, handle))
            elif op == RELEASE:
                h.release((node, handle))
            elif op == CREATE_REQ:
                r["handle"] = h.create_request()[1]
            elif op == HANDLE_REQ:
                r["handle"] = h.handle_request((0, handle))[1]
            else:
                h.handle_response((peer, handle), t)
        except amd.LbftError as e:
            if e.code != -5:
                raise
            r["status"] = -5
        want = self.host.call(op, inst, node, peer, handle, t)
        assert r == want, ("device != host build", op, node, r, want)
        return r

    def view(self, inst, node):
        return self.nodes[node].view()

    def save_node(self, inst, node):
        try:
            return self.nodes[node].save_node()
        except self.amd.LbftError as e:
            assert e.code == -3
            return None

    def end(self, n):
        res = self.sim.manual_finalize()
        assert res.faults[0] == 0
        out = []
        for k in range(n):
            hist = res.committed_history(0, k)
            out.append(dict(view=self.view(0, k), commit_count=int(res.commit_counts[0, k]), history=hist,
                            last_state=int(res.last_committed_states[0, k]), image=self.save_node(0, k),
                            record_hashes=np.array([[int(x["block_hash"]), int(x["state"]), int(x["qc_hash"]), int(x["num_votes"])]
                                                    for x in res.committed_record_hashes(0, k)], dtype=np.uint64).reshape(-1, 4)))
        return out


# drawn sessions replayed one call per launch: a subset, plus the large networks with request / response at 33, 65 and 128 nodes
DEVICE_SEEDS = [1, 5, 8, 11, 12, 13]
DEVICE_EXCHANGE_BIG = [(33, 1001), (65, 1003), (128, 1005)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed", [(None, s) for s in DEVICE_SEEDS] + DEVICE_EXCHANGE_BIG)
def test_device_single_calls_equal_the_oracle(oracle, n, seed):
    import librabft_simulator_amd as amd
    spec = draw_spec(seed, n=n, exchange_big=n is not None)
    dev = DeviceSingle(amd, oracle, spec)
    ora = OracleSide(oracle, spec)
    stats = new_stats()
    drive_single(dev, 0, ora, spec, stats, dev.host.caps["scap"])
    compare_end(dev.end(spec["n"]), ora, spec, stats)
    assert stats["calls"] > 300


def batched_sessions(amd, oracle, spec, m, lanes_per_wavefront, rng):
    """m instances, each with its own session (seed spec.seed + i), advanced through lbft_node_calls: every launch carries the next call
    of a random subset of the instances (the first launch: all of them)."""
    from librabft_simulator_amd import _lib
    sim, nodes = device_batch(amd, spec, [spec["seed"] + i for i in range(m)], lanes_per_wavefront=lanes_per_wavefront)
    specs = [dict(spec, seed=spec["seed"] + i) for i in range(m)]
    oras = [OracleSide(oracle, s) for s in specs]
    gens = [session(s, new_stats()) for s in specs]
    pending = [g.send(None) for g in gens]
    ops_seen, launches, biggest = set(), 0, 0
    while any(p is not None for p in pending):
        idle = [i for i in range(m) if pending[i] is not None and pending[i][0] == "save"]
        for i in idle:  # (save_node images outside the launches)
            k = pending[i][1]
            try:
                img = sim.save_node(i, k)
                assert img == oras[i].sim.save_node(k), (i, k)
            except amd.LbftError as e:
                assert e.code == -3
            pending[i] = next(gens[i], None)
        live = [i for i in range(m) if pending[i] is not None]
        if not live:
            break
        pick = live if launches == 0 else [i for i in live if rng.random() < 0.7] or live[:1]
        calls = [pending[i] for i in pick]
        res = sim.node_calls([model_args(c)[:1] + (i,) + model_args(c)[1:] for i, c in zip(pick, calls)])
        launches += 1
        biggest = max(biggest, len(pick))
        for i, c, got in zip(pick, calls, res):
            ops_seen.add(c[0])
            out = check_result(c, got, oras[i].call(*c), 1)
            out["round_moved"] = out["changed"] = False
            try:
                pending[i] = gens[i].send(out)
            except StopIteration:
                pending[i] = None
        for i in rng.sample(pick, min(3, len(pick))):  # sampled views of the touched nodes
            k = touched(calls[pick.index(i)])
            if k is not None:
                assert nodes[i][k].view() == oras[i].sim.node_view(k), (i, k)
    res = sim.manual_finalize()
    assert not res.faults.any()
    for i in rng.sample(range(m), min(m, 12)):
        for k in range(spec["n"]):
            assert nodes[i][k].view() == oras[i].sim.node_view(k)
            hist = oras[i].sim.committed_history(k)
            assert int(res.commit_counts[i, k]) == len(hist) and (res.committed_history(i, k) == hist).all()
            assert int(res.last_committed_states[i, k]) == oras[i].sim.last_committed_states()[k]
    return ops_seen, launches, biggest


@pytest.mark.gpu
@pytest.mark.parametrize("lanes_per_wavefront", [0, 8])
def test_device_batched_sessions_equal_the_oracle(oracle, lanes_per_wavefront):
    import librabft_simulator_amd as amd
    rng = random.Random(lanes_per_wavefront)
    spec = dict(draw_spec(13, n=5, quirks=1), steps=150, equivocate_every=0)
    m = 1100 if lanes_per_wavefront == 0 else 203  # (not multiples of 64; > 1 024 calls in the first launch)
    ops, launches, biggest = batched_sessions(amd, oracle, spec, m, lanes_per_wavefront, rng)
    assert ops == set(range(7)), ops
    assert biggest == m and launches > 100
    print("batched node-level sessions: %d instances, %d launches" % (m, launches))


class DeviceInst:
    """The calls of instance 1 of a device batch through lbft_node_calls (raw ABI, so that per-result statuses are seen), instance 0
    getting an update in the same launch."""
    def __init__(self, made):
        self.amd, self.sim, self.nodes, self.ora0 = made
        self.hs = None

    def call(self, op, node, peer, handle, t):
        from librabft_simulator_amd import _lib
        arr = (_lib.LbftNodeCall * 2)(_lib.LbftNodeCall(op, 1, node, peer, handle, 0, t), _lib.LbftNodeCall(0, 0, 0, 0, 0, 0, 7))
        res = (_lib.LbftNodeResult * 2)()
        rc = _lib.lib().lbft_node_calls(self.sim._h, arr, 2, res)
        r = res[0]
        assert rc == (-5 if r.status else 0)
        a = res[1].actions.as_dict()
        assert res[1].status == 0 and a == self.ora0.sim.node_update(0, 7)  # the other result of the launch
        return {"actions": r.actions.as_dict() if op == UPDATE else None, "handle": int(r.handle), "should_sync": bool(r.should_sync),
                "status": int(r.status)}

    def view(self, node):
        return self.nodes[1][node].view()


@pytest.mark.gpu
def test_device_snapshot_pool_single_and_batched(oracle):
    import librabft_simulator_amd as amd
    spec = dict(draw_spec(5, n=4, quirks=1), equivocate_every=0)

    class Single(HostInst):
        def __init__(self, made):
            self.sim, self.nodes = made
            self.hs = None

        def call(self, op, node, peer, handle, t):
            return DeviceSingle.call(self, op, 0, node, peer, handle, t)

        def view(self, node):
            return self.nodes[node].view()

    def make_single():
        sim, nodes = device_batch(amd, spec, [spec["seed"]], POOL_CAP)
        host = oracle.HostSession(oracle_config(oracle, spec), [spec["seed"]], spec["max_clock"], oracle.manual_caps(4, 1, spec["max_clock"], POOL_CAP))
        return sim, nodes[0], host

    class SingleShadow(Single):
        def __init__(self, made):
            self.sim, self.nodes, self.host = made
            self.amd, self.hs = amd, None

    stats, _ = run_pool_session(oracle, make_single, spec, wrap=SingleShadow)
    assert stats["full_at"] == POOL_CAP

    ora0 = OracleSide(oracle, dict(spec, seed=spec["seed"]))

    def make_batched():
        sim, nodes = device_batch(amd, spec, [spec["seed"], spec["seed"]], POOL_CAP)
        return amd, sim, nodes, ora0
    stats, _ = run_pool_session(oracle, make_batched, spec, wrap=DeviceInst)
    assert stats["full_at"] == POOL_CAP


@pytest.mark.gpu
def test_device_refusals_before_any_launch(oracle):
    import librabft_simulator_amd as amd
    from librabft_simulator_amd import _lib
    ref = dict(draw_spec(3, n=4, quirks=0), equivocate_every=0, keep_stores=False)
    sim, nodes = device_batch(amd, ref, [1, 2])
    for op in (_lib.CALL_CREATE_REQUEST, _lib.CALL_HANDLE_REQUEST, _lib.CALL_HANDLE_RESPONSE):
        with pytest.raises(amd.LbftError) as e:
            sim.node_calls([(op, 0, 0, 0, 0, 1)])
        assert e.value.code == -3
    scap = oracle.manual_caps(4, 0, ref["max_clock"])["scap"]  # (the session's snapshot pool: handles at and past it are refused)
    for op in (_lib.CALL_HANDLE_NOTIFICATION, _lib.CALL_RELEASE_NOTIFICATION):
        with pytest.raises(amd.LbftError) as e:
            sim.node_calls([(op, 0, 1, 0, scap, 1)])
        assert e.value.code == -1
    with pytest.raises(amd.LbftError) as e:
        sim.node_calls([(_lib.CALL_UPDATE_NODE, 1, 0, 0, 0, 1), (_lib.CALL_UPDATE_NODE, 1, 2, 0, 0, 1)])
    assert e.value.code == -1


@pytest.mark.gpu
def test_device_node_time_contract(oracle):
    """0 <= node_time <= LBFT_MAX_CLOCK: times at and past the session's max_clock equal the oracle; outside, every node-level call that
    takes a time refuses with LBFT_ERR_INVALID before any launch and leaves the node untouched.  (lbft_batch_load_node only compares its
    node_time with the image's times and takes any value.)"""
    import librabft_simulator_amd as amd
    from librabft_simulator_amd import _lib
    spec = dict(draw_spec(11, n=4, quirks=1), max_clock=1000, equivocate_every=0, keep_stores=False)
    sim, nodes = device_batch(amd, spec, [11, 12])
    ora = OracleSide(oracle, spec)
    for t in (999, 1000, 1001, 5 * 10 ** 5):
        for k in range(4):
            assert nodes[0][k].update_node(t) == ora.call(UPDATE, k, 0, None, t)["actions"]
    before = [nodes[0][k].view() for k in range(4)]
    img = sim.save_node(0, 0)
    req = nodes[0][1].create_request()
    resp = nodes[0][0].handle_request(req)
    for bad in (-1, LBFT_MAX_CLOCK + 1, 1 << 40, -(1 << 62)):
        for fn in (lambda: nodes[0][0].update_node(bad), lambda: nodes[0][1].handle_response(resp, bad),
                   lambda: sim.node_calls([(_lib.CALL_UPDATE_NODE, 0, 0, 0, 0, bad)]),
                   lambda: sim.node_calls([(_lib.CALL_UPDATE_NODE, 1, 0, 0, 0, 5), (_lib.CALL_HANDLE_RESPONSE, 0, 1, 0, resp[1], bad)])):
            with pytest.raises(amd.LbftError) as e:
                fn()
            assert e.value.code == -1
    assert [nodes[0][k].view() for k in range(4)] == before and sim.save_node(0, 0) == img
    sim.load_node(0, 0, img, 1 << 40)
    assert nodes[0][0].view() == before[0] and sim.save_node(0, 0) == img
    ref = nodes[1][0].update_node(5)  # (instance 1 untouched as well: its first update is still the oracle's first)
    assert ref == OracleSide(oracle, dict(spec, seed=12)).call(UPDATE, 0, 0, None, 5)["actions"]
    for t in (LBFT_MAX_CLOCK - 100, LBFT_MAX_CLOCK):
        for k in range(4):
            assert nodes[0][k].update_node(t) == ora.call(UPDATE, k, 0, None, t)["actions"]
            assert nodes[0][k].view() == ora.sim.node_view(k)
