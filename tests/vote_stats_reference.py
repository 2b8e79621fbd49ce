"""The vote statistics (lbft_batch_vote_stats, include/lbft.h) restated in plain Python / numpy over oracle data only: the blocks and
quorum certificates of every node's save_node image (the current and the past record stores, read with bincode_nodestate and united by
hash), committed_record_hashes of the reference node for the chain, the commit counts, the fault words and the groups.  Test
infrastructure: nothing here comes from csrc/ or the package.

What it relies on is asserted: a certified block has ONE voter set across all nodes' images, and that set has as many voters as the
record hashes' num_votes says."""
import numpy as np

import bincode_nodestate

FAMILIES = ("votes", "weight", "margin", "skipped", "blocks", "orphaned", "pending", "certified_off_chain")
VOTES, WEIGHT, MARGIN, SKIPPED, BLOCKS, ORPHANED, PENDING, CERTIFIED_OFF = range(8)
VOTE_STATS = 4 * len(FAMILIES)
PROPOSED, COL_ORPHANED, VOTED = range(3)
NODE_COLUMNS = 3


def quorum_of(rights):
    return 2 * sum(int(w) for w in rights) // 3 + 1


def pool_of(sim, n):
    """The oracle's blocks and certificates of one instance: ({block hash: (epoch, round, author)}, {block hash: sorted voters})."""
    blocks, voters = {}, {}
    for q in range(n):
        image = bincode_nodestate.node_state(sim.save_node(q))
        for store in [image["record_store"]] + [s for _, s in image["past_record_stores"]]:
            epoch = store["epoch_id"]
            for h, b in store["blocks"]:
                entry = (epoch, b["round"], b["author"])
                assert blocks.setdefault(h, entry) == entry, "one hash, two blocks"
            for _, qc in store["quorum_certificates"]:
                v = tuple(sorted(a for a, _ in qc["votes"]))
                assert len(set(v)) == len(v) and v, "a certificate's voters are distinct and not empty"
                assert voters.setdefault(qc["certified_block_hash"], v) == v, "one voter set per certified block across all nodes"
    assert set(voters) <= set(blocks), "a certificate of no block"
    return blocks, voters


def instance(sim, n, rights=None, rotation=0):
    """The samples of one finished OracleSim: the four per-entry families as lists, the four per-instance counts, the chain length,
    the vote-count histogram [n + 1] and the node table [n, 3]."""
    rights = [1] * n if rights is None else [int(w) for w in rights]
    quorum = quorum_of(rights)
    blocks, voters = pool_of(sim, n)
    counts = sim.commit_counts()
    ref = int(np.argmax(counts))  # (the lowest-numbered node with the most commits)
    hashes = sim.committed_record_hashes(ref)
    chain = [int(h) for h in hashes["block_hash"]]
    assert len(chain) == counts[ref] and len(set(chain)) == len(chain) and set(chain) <= set(blocks)
    out = {"votes": [], "weight": [], "margin": [], "skipped": [], "length": len(chain), "votes_hist": np.zeros(n + 1, dtype=np.uint64),
           "nodes": np.zeros((n, NODE_COLUMNS), dtype=np.uint64)}
    for k, h in enumerate(chain):
        epoch, rnd, _ = blocks[h]
        v = [a for a in voters.get(h, ()) if a < n]
        assert len(voters.get(h, ())) == int(hashes["num_votes"][k]), "len(votes) == num_votes of the record hashes"
        if v:
            weight = sum(rights[(a + epoch * rotation) % n] for a in v)
            assert weight >= quorum
            out["votes"].append(len(v)); out["weight"].append(weight); out["margin"].append(weight - quorum)
            out["votes_hist"][len(v)] += 1
            for a in v:
                out["nodes"][a, VOTED] += 1
        if k > 0 and blocks[chain[k - 1]][0] == epoch:
            assert rnd > blocks[chain[k - 1]][1], "chain rounds rise strictly within an epoch"
            out["skipped"].append(rnd - blocks[chain[k - 1]][1] - 1)
    on_chain = set(chain)
    tip = blocks[chain[-1]][:2] if chain else None
    orphaned = pending = certified_off = 0
    for h, (epoch, rnd, author) in blocks.items():
        out["nodes"][author, PROPOSED] += 1
        if h in on_chain:
            continue
        if tip is not None and (epoch, rnd) <= tip:
            orphaned += 1
            out["nodes"][author, COL_ORPHANED] += 1
        else:
            pending += 1
        certified_off += 1 if [a for a in voters.get(h, ()) if a < n] else 0
    out.update(blocks=len(blocks), orphaned=orphaned, pending=pending, certified_off_chain=certified_off)
    assert out["blocks"] == out["length"] + orphaned + pending
    return out


def group(instances, faults=None, set_of=None, groups=1):
    """Per group: the eight families as lists of samples, the vote-count histogram and the node table, over the instances without a
    fault (`instances`: what instance() gave, or None for one that is skipped anyway)."""
    out = []
    for g in range(groups):
        fam, votes_hist, nodes = [[] for _ in FAMILIES], None, None
        for i, inst in enumerate(instances):
            if (set_of is not None and int(set_of[i]) != g) or (faults is not None and int(faults[i]) != 0):
                continue
            for f in (VOTES, WEIGHT, MARGIN, SKIPPED):
                fam[f] += inst[FAMILIES[f]]
            for f in (BLOCKS, ORPHANED, PENDING, CERTIFIED_OFF):
                fam[f].append(inst[FAMILIES[f]])
            votes_hist = inst["votes_hist"].copy() if votes_hist is None else votes_hist + inst["votes_hist"]
            nodes = inst["nodes"].copy() if nodes is None else nodes + inst["nodes"]
        out.append((fam, votes_hist, nodes))
    return out


def bin_votes(grouped, n, width, bins):
    """group()'s result as the call's four arrays: margin_hist [groups, bins], votes_hist [groups, n + 1], node_table [groups, n, 3],
    stats [groups, 32]."""
    groups = len(grouped)
    margin = np.zeros((groups, bins), dtype=np.uint64)
    votes = np.zeros((groups, n + 1), dtype=np.uint64)
    nodes = np.zeros((groups, n, NODE_COLUMNS), dtype=np.uint64)
    stats = np.zeros((groups, VOTE_STATS), dtype=np.uint64)
    for g, (fam, votes_hist, node_table) in enumerate(grouped):
        for f, samples in enumerate(fam):
            if samples:
                stats[g, 4 * f:4 * f + 4] = (len(samples), sum(samples), min(samples), max(samples))
        for v in fam[MARGIN]:
            margin[g, min(v // width, bins - 1)] += 1
        if votes_hist is not None:
            votes[g], nodes[g] = votes_hist, node_table
    return margin, votes, nodes, stats


def default_binning(rights, n):
    rights = [1] * n if rights is None else rights
    total = sum(int(w) for w in rights)
    return 1, min(total - quorum_of(rights) + 1, 4096)


def identities(margin, votes, nodes, stats, lengths_sum=None, unit=True):
    """What holds on every result: the histograms sum to their families' sample counts, the node table's columns to the families' sums,
    blocks = chain length + orphaned + pending (lengths_sum: the sum of the clean instances' chain lengths, when the caller has it)."""
    s = stats.astype(np.int64)
    assert (margin.sum(axis=1) == s[:, 4 * MARGIN]).all() and (votes.sum(axis=1) == s[:, 4 * VOTES]).all()
    assert (s[:, 4 * VOTES] == s[:, 4 * WEIGHT]).all() and (s[:, 4 * VOTES] == s[:, 4 * MARGIN]).all()
    assert ((votes * np.arange(votes.shape[1], dtype=np.uint64)).sum(axis=1) == s[:, 4 * VOTES + 1]).all()
    assert (nodes[:, :, PROPOSED].sum(axis=1) == s[:, 4 * BLOCKS + 1]).all()
    assert (nodes[:, :, COL_ORPHANED].sum(axis=1) == s[:, 4 * ORPHANED + 1]).all()
    assert (nodes[:, :, VOTED].sum(axis=1) == s[:, 4 * VOTES + 1]).all()
    if unit:
        assert (nodes[:, :, VOTED].sum(axis=1) == s[:, 4 * WEIGHT + 1]).all()
    if lengths_sum is not None:
        assert (s[:, 4 * BLOCKS + 1] == np.asarray(lengths_sum) + s[:, 4 * ORPHANED + 1] + s[:, 4 * PENDING + 1]).all()
