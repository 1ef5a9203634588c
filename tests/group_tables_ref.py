"""Plain NumPy restatement of the group tables bff_group_components writes (include/bff_hip.h), and the random
component structures the tests feed it.  No GPU, no library: tests/test_host_logic.py checks this reference
against projection.component_csr and the native host twin, tests/test_gpu_device_groups.py checks the device
against it."""
import numpy as np

SLICE = 32          # members per work item of bff_or_reduce_grouped


def group_tables_ref(comp, area, thr, min_members, cap):
    """comp: flattened component ids (comp[i] = smallest member of i's component), area: int per row.
    -> dict(info [4], K, sizes, first, offs [min(K, cap) + 1], members, slices [info[3]][3] (group, lo, hi))."""
    comp = np.asarray(comp, dtype=np.int64)
    area = np.asarray(area, dtype=np.int64)
    n = comp.shape[0]
    idx = np.arange(n)
    roots = idx[comp == idx]                                   # ascending = the groups' order
    size = np.bincount(comp, minlength=n)[roots] if n else np.zeros(0, np.int64)
    loops = bool(np.float32(1) > np.float32(thr))
    void = (size == 1) & ~((area[roots] > 0) & loops)
    kept = ~void & (size >= max(min_members, 1))
    kr, ks = roots[kept], size[kept]
    big_k = int(kr.size)
    k = min(big_k, cap)
    n_slices = int(((ks[:k] + SLICE - 1) // SLICE).sum())
    flags = (1 if big_k > cap else 0) | (2 if (min_members <= 0 and void.any()) else 0)
    info = np.array([big_k, flags, int(ks.max()) if big_k else 0, n_slices], np.int64)
    offs = np.zeros(k + 1, np.int64)
    np.cumsum(ks[:k], out=offs[1:])
    order = np.argsort(comp, kind="stable")                    # members ascending inside a component
    start = np.searchsorted(comp[order], kr[:k])
    members = np.concatenate([order[s:s + z] for s, z in zip(start, ks[:k])]) if k else np.zeros(0, np.int64)
    slices = [(g, lo, min(lo + SLICE, offs[g + 1])) for g in range(k) for lo in range(offs[g], offs[g + 1], SLICE)]
    return {"info": info, "K": big_k, "sizes": ks[:k], "first": kr[:k], "offs": offs, "members": members,
            "slices": np.array(slices, np.int64).reshape(-1, 3)}


def build_components(rng, n, k_goal, special, thr, min_members, alive_singles, tree="random"):
    """Random components over n rows with exactly k_goal kept groups: the `special` group sizes (each >= 2), fillers of
    size max(min_members, 2) .. +2, the rest singletons, `alive_singles` of them with area > 0.  Members are scattered
    over the whole index range.  -> (parent, comp, area): parent is a disjoint-set forest whose root is the smallest
    member and parent[i] < i inside a component ("chain": every member hangs under the previous one, the deepest
    forest; "random": under a random smaller member)."""
    need = max(min_members, 1)
    loops = bool(np.float32(1) > np.float32(thr))
    sizes = list(special)
    assert all(s >= 2 for s in sizes)
    kept_single = alive_singles if (loops and need <= 1) else 0
    fill = k_goal - sum(s >= need for s in sizes) - kept_single
    assert fill >= 0, (k_goal, special)
    sizes += [max(need, 2) + int(rng.integers(0, 3)) for _ in range(fill)]
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    assert sum(sizes) + alive_singles <= n, (n, sum(sizes), alive_singles)
    perm = rng.permutation(n)
    parent = np.arange(n, dtype=np.int64)
    area = np.zeros(n, np.int64)
    st = 0
    for s in sizes:
        m = np.sort(perm[st:st + s])
        st += s
        if tree == "chain":
            parent[m[1:]] = m[:-1]
        else:
            parent[m[1:]] = m[(rng.random(s - 1) * np.arange(1, s)).astype(np.int64)]
        area[m] = rng.integers(0, 50, s)                       # a group's root may be empty: it is kept anyway
    singles = perm[st:]
    area[singles[:alive_singles]] = rng.integers(1, 100, alive_singles)
    comp = parent.copy()
    while True:                                                # flatten: parent[i] < i, so this ends
        nxt = comp[comp]
        if np.array_equal(nxt, comp):
            break
        comp = nxt
    return parent.astype(np.int32), comp.astype(np.int32), area.astype(np.int32)
