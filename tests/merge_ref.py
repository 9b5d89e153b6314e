"""A plain restatement of generateMatchesExhaustive's merge (src/MatchFactory.cu:943-1020; include/ssrlcv_hip.h, "Host half
of generateMatchesExhaustive"), written from the description and not from csrc/host_merge.cpp or
csrc/merge.hip: one real Python list per (image, feature), appended to in pair order, intersected as Python sets, emptied
with list.clear(), records appended as the seeds are accepted.  No CSR, no live lengths, no outcome table.

    every image but the last owns one list per feature; the pair (q, t) appends (t, target) to the list of (q, query)
    for every seed feature of images 0 .. V-3, in order, whose list is not empty:
        prev = the seed's list
        loop: head = prev[0]; stop if head is in the last image; next = head's list; stop if next is empty;
              REJECT unless every entry of next is in prev; stop if next has one entry; prev = next
        rejected: the seed's list is emptied
        accepted: MultiMatch{1 + len(list), index of its first member}, members = the seed, then its list;
                  the lists of all members but the last are emptied, up to the first member in the last image

`mutant` turns one clause of that into a plausible mistake (tests/test_merge_cases.py shows that the cases notice each)."""
import numpy as np

PAIR = np.dtype([("a", "<u4", (2,)), ("b", "<u4", (2,))])

MUTANTS = ("never_continue", "follow_last", "compare_with_prev", "no_clear_on_accept", "clear_last_member_too",
           "no_stop_at_last_image")


def merge_ref(num_features, blocks, reverse=False, mutant=None):
    """-> (mm uint32 [n, 2] = {numKeyPoints, index}, members uint32 [m, 2] = {image, feature}, stats).
    reverse = True visits the seeds of each image from the last feature to the first (the records then come in that order).
    stats: good, bad, skipped_because_cleared, deep, max_depth, ge4 (see the issue these cases were built for: a "deep" seed
    took at least one further hop, depth = number of hops), live_images = seed images that had a non-empty seed at their
    turn, outcome = {(image, feature): "good" | "bad" | "skipped"} of every seed that had a list to begin with."""
    assert mutant is None or mutant in MUTANTS, mutant
    V = len(num_features)
    lists = [[[] for _ in range(int(num_features[i]))] for i in range(V - 1)]  # the last image owns none
    for blk in blocks:
        for (qi, qf), (ti, tf) in zip(blk["a"].tolist(), blk["b"].tolist()):
            lists[qi][qf].append((ti, tf))
    had_list = [[bool(l) for l in img] for img in lists]
    mm, members, outcome = [], [], {}
    stats = dict(good=0, bad=0, skipped_because_cleared=0, deep=0, max_depth=0, ge4=0, live_images=0)
    for i in range(V - 2):
        order = range(len(lists[i]))
        live = False
        for f in (reversed(order) if reverse else order):
            seed = lists[i][f]
            if not seed:
                if had_list[i][f]:
                    stats["skipped_because_cleared"] += 1
                    outcome[(i, f)] = "skipped"
                continue
            live = True
            prev, depth, accepted = seed, 0, True
            while True:
                head = prev[-1] if mutant == "follow_last" else prev[0]
                if head[0] == V - 1:
                    break
                nxt = lists[head[0]][head[1]]
                if not nxt:
                    break
                if len(set(prev) & set(nxt)) != len(prev if mutant == "compare_with_prev" else nxt):
                    accepted = False
                    break
                if len(nxt) == 1 or mutant == "never_continue":
                    break
                prev = nxt
                depth += 1
            stats["deep"] += depth > 0
            stats["max_depth"] = max(stats["max_depth"], depth)
            if not accepted:
                stats["bad"] += 1
                outcome[(i, f)] = "bad"
                seed.clear()
                continue
            stats["good"] += 1
            stats["ge4"] += len(seed) + 1 >= 4
            outcome[(i, f)] = "good"
            mm.append((len(seed) + 1, len(members)))
            members.append((i, f))
            members.extend(seed)
            if mutant == "no_clear_on_accept":
                continue
            for m in (list(seed) if mutant == "clear_last_member_too" else seed[:-1]):
                if m[0] == V - 1 and mutant != "no_stop_at_last_image":
                    break
                lists[m[0]][m[1]].clear()  # (the mutant reaches for a list of the last image: there is none, IndexError)
        stats["live_images"] += live
    stats["outcome"] = outcome
    return (np.array(mm, np.uint32).reshape(-1, 2), np.array(members, np.uint32).reshape(-1, 2), stats)


def order_dependent(num_features, blocks):
    """Seeds whose outcome differs between walking each image's seeds first to last and last to first."""
    fwd = merge_ref(num_features, blocks)[2]["outcome"]
    bwd = merge_ref(num_features, blocks, reverse=True)[2]["outcome"]
    return sum(fwd.get(k) != bwd.get(k) for k in set(fwd) | set(bwd))
