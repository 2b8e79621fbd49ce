"""The epoch statistics (lbft_batch_epoch_stats, include/lbft.h) restated in plain Python / numpy over oracle data only: the blocks of
every node's save_node image (the current and the past record stores, read with bincode_nodestate and united by hash) with their
store's epoch_id and their own round, author and time, committed_record_hashes of the reference node for the chain, the commit counts,
the startup times, the nodes' epochs, the fault words and the groups.  Test infrastructure: nothing here comes from csrc/ or the
package."""
import numpy as np

import bincode_nodestate

FAMILIES = ("segments", "node_epoch", "behind", "length", "duration", "last_round", "first_round", "handover", "stranded", "blocks")
SEGMENTS, NODE_EPOCH, BEHIND, LENGTH, DURATION, LAST_ROUND, FIRST_ROUND, HANDOVER, STRANDED, BLOCKS = range(10)
EPOCH_STATS = 4 * len(FAMILIES)
COLUMNS = ("segments", "complete", "entries", "duration", "handover", "stranded", "blocks")
COL_SEGMENTS, COL_COMPLETE, COL_ENTRIES, COL_DURATION, COL_HANDOVER, COL_STRANDED, COL_BLOCKS = range(7)
MAX_BINS = 512


def pool_of(sim, n):
    """The oracle's blocks of one instance: {block hash: (epoch, round, author, time)}."""
    blocks = {}
    for q in range(n):
        image = bincode_nodestate.node_state(sim.save_node(q))
        for store in [image["record_store"]] + [s for _, s in image["past_record_stores"]]:
            for h, b in store["blocks"]:
                entry = (int(store["epoch_id"]), int(b["round"]), int(b["author"]), int(b["time"]))
                assert blocks.setdefault(h, entry) == entry, "one hash, two blocks"
    return blocks


def samples(chain, blocks, node_epochs):
    """One instance from its chain [(epoch, round, global proposal time)], its pool `blocks` = [(epoch, on the chain)] and its nodes'
    epochs: the ten families as lists and the table's contributions as [(epoch, column, value)]."""
    fam = [[] for _ in FAMILIES]
    cells = []
    e_max = max(node_epochs)
    fam[NODE_EPOCH] = [int(e) for e in node_epochs]
    fam[BEHIND] = [int(e_max - e) for e in node_epochs]
    segments = []  # [first index, last index] of every maximal run of one epoch
    for k, (e, _, _) in enumerate(chain):
        if k and chain[k - 1][0] == e:
            segments[-1][1] = k
        else:
            segments.append([k, k])
    fam[SEGMENTS] = [len(segments)]
    for q, (a, b) in enumerate(segments):
        e = chain[a][0]
        cells += [(e, COL_SEGMENTS, 1), (e, COL_ENTRIES, b - a + 1)]
        fam[FIRST_ROUND].append(chain[a][1])
        if q + 1 < len(segments):  # complete
            duration = max(chain[b][2] - chain[a][2], 0)
            fam[LENGTH].append(b - a + 1); fam[DURATION].append(duration); fam[LAST_ROUND].append(chain[b][1])
            cells += [(e, COL_COMPLETE, 1), (e, COL_DURATION, duration)]
        if q:  # the boundary before it
            handover = max(chain[a][2] - chain[a - 1][2], 0)
            fam[HANDOVER].append(handover)
            cells.append((e, COL_HANDOVER, handover))
    stranded = 0
    for e, member in blocks:
        cells.append((e, COL_BLOCKS, 1))
        if chain and not member and e < chain[-1][0]:
            stranded += 1
            cells.append((e, COL_STRANDED, 1))
    fam[STRANDED], fam[BLOCKS] = [stranded], [len(blocks)]
    return {"families": fam, "cells": cells, "length": len(chain)}


def instance(sim, n):
    """samples() of one finished OracleSim."""
    blocks = pool_of(sim, n)
    counts = sim.commit_counts()
    ref = int(np.argmax(counts))  # (the lowest-numbered node with the most commits)
    chain_hashes = [int(h) for h in sim.committed_record_hashes(ref)["block_hash"]]
    assert len(chain_hashes) == counts[ref] and len(set(chain_hashes)) == len(chain_hashes) and set(chain_hashes) <= set(blocks)
    startup = [int(t) for t in sim.startup_times()]
    chain = [(blocks[h][0], blocks[h][1], startup[blocks[h][2]] + blocks[h][3]) for h in chain_hashes]
    on_chain = set(chain_hashes)
    out = samples(chain, [(b[0], h in on_chain) for h, b in blocks.items()], [int(e) for e in sim.epochs()])
    out["node_epochs"] = [int(e) for e in sim.epochs()]
    return out


def group(instances, faults=None, set_of=None, groups=1):
    """Per group (families as lists of samples, table cells) over the instances without a fault."""
    out = []
    for g in range(groups):
        fam, cells = [[] for _ in FAMILIES], []
        for i, inst in enumerate(instances):
            if (set_of is not None and int(set_of[i]) != g) or (faults is not None and int(faults[i]) != 0):
                continue
            for f in range(len(FAMILIES)):
                fam[f] += inst["families"][f]
            cells += inst["cells"]
        out.append((fam, cells))
    return out


def bin_epochs(grouped, width, bins, epoch_bins):
    """group()'s result as the call's three arrays: handover_hist [groups, bins], epoch_table [groups, epoch_bins, 7], stats [groups, 40]."""
    groups = len(grouped)
    hist = np.zeros((groups, bins), dtype=np.uint64)
    table = np.zeros((groups, epoch_bins, len(COLUMNS)), dtype=np.uint64)
    stats = np.zeros((groups, EPOCH_STATS), dtype=np.uint64)
    for g, (fam, cells) in enumerate(grouped):
        for f, s in enumerate(fam):
            if s:
                stats[g, 4 * f:4 * f + 4] = (len(s), sum(s), min(s), max(s))
        for v in fam[HANDOVER]:
            hist[g, min(v // width, bins - 1)] += 1
        for e, c, v in cells:
            table[g, min(e, epoch_bins - 1), c] += np.uint64(v)
    return hist, table, stats


def default_binning(max_clock, width=None, bins=None):
    """BatchResult.epoch_stats' defaults: [0, max_clock] in at most 4 096 bins."""
    span = max_clock + 1
    if width is None:
        width = -(-span // (bins if bins else 4096))
    if bins is None:
        bins = -(-span // width)
    return width, bins


def identities(hist, table, stats, lengths_sum=None, with_chain=None):
    """What holds on every result (include/lbft.h): each column of the table summed over its rows equals the matching family's sum or
    sample count; entries sum to the clean instances' chain lengths (lengths_sum, per group, when the caller has it); boundaries =
    segments - the instances with a chain (with_chain, per group, when the caller has it)."""
    s = stats.astype(np.int64)
    col = table.astype(np.int64).sum(axis=1)
    assert (hist.sum(axis=1) == s[:, 4 * HANDOVER]).all()
    assert (col[:, COL_SEGMENTS] == s[:, 4 * FIRST_ROUND]).all() and (col[:, COL_SEGMENTS] == s[:, 4 * SEGMENTS + 1]).all()
    assert (col[:, COL_COMPLETE] == s[:, 4 * LENGTH]).all() and (s[:, 4 * LENGTH] == s[:, 4 * DURATION]).all() and (s[:, 4 * LENGTH] == s[:, 4 * LAST_ROUND]).all()
    assert (col[:, COL_DURATION] == s[:, 4 * DURATION + 1]).all() and (col[:, COL_HANDOVER] == s[:, 4 * HANDOVER + 1]).all()
    assert (col[:, COL_STRANDED] == s[:, 4 * STRANDED + 1]).all() and (col[:, COL_BLOCKS] == s[:, 4 * BLOCKS + 1]).all()
    assert (col[:, COL_ENTRIES] >= s[:, 4 * LENGTH + 1]).all() and (s[:, 4 * NODE_EPOCH] == s[:, 4 * BEHIND]).all()
    assert (s[:, 4 * SEGMENTS] == s[:, 4 * STRANDED]).all() and (s[:, 4 * SEGMENTS] == s[:, 4 * BLOCKS]).all()
    if lengths_sum is not None:
        assert (col[:, COL_ENTRIES] == np.asarray(lengths_sum)).all()
    if with_chain is not None:
        assert (s[:, 4 * HANDOVER] == s[:, 4 * FIRST_ROUND] - np.asarray(with_chain)).all()
