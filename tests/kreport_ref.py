"""A plain-Python restatement of include/kslam_kreport.h: the rows and the six-column file from the taxDB text and the taxonomy
ids, with a dict tree and recursion -- no code shared with the host twin (host/kreport.cpp) or the kernels (csrc/kreport.hip) --
and the seam cases tests/test_kreport_ref.py and tests/test_gpu_kreport.py run."""
import collections

import numpy as np

NO_NODE = 0xFFFFFFFF
ROW_DT = np.dtype([("tax_id", "<u4"), ("node", "<u4"), ("direct", "<u8"), ("clade", "<u8")])
LETTER = {b"superkingdom": "D", b"domain": "D", b"kingdom": "K", b"phylum": "P", b"class": "C", b"order": "O", b"family": "F",
          b"genus": "G", b"species": "S"}


def tax_text(records):
    """[(id, parent, name, rank), ...] -> the taxDB text: four lines per record"""
    return b"".join(b"%d\n%d\n%s\n%s\n" % (i, p, n.encode() if isinstance(n, str) else n, r.encode() if isinstance(r, str) else r)
                    for i, p, n, r in records)


class Tree:
    """the forest of include/kslam_taxonomy.h: nodes in file order (a repeated id keeps its first record), then one node per
    parent id the file mentions but never defines, in the order of their first mention (parent 1, empty name and rank)"""

    def __init__(self, text):
        lines = text.split(b"\n")
        if lines and lines[-1] == b"":
            lines.pop()
        assert len(lines) % 4 == 0
        self.order, self.parent, self.name, self.rank = [], {}, {}, {}
        for k in range(0, len(lines), 4):
            i, p = int(lines[k]), int(lines[k + 1])
            if i in self.parent:
                continue
            self.order.append(i)
            self.parent[i], self.name[i], self.rank[i] = p, lines[k + 2], lines[k + 3]
        for i in list(self.order):
            p = self.parent[i]
            if p not in (0, 1) and p not in self.parent:
                self.order.append(p)
                self.parent[p], self.name[p], self.rank[p] = 1, b"", b""
        self.node = {i: n for n, i in enumerate(self.order)}
        self.kids = collections.defaultdict(list)
        for i in self.order:
            if self.parent[i] not in (0, 1):
                self.kids[self.parent[i]].append(i)

    def top(self, i):
        return self.parent[i] in (0, 1)


def _counts(tree, ids):
    direct = collections.Counter(int(x) for x in np.asarray(ids).tolist() if x)
    clade = {}

    def below(i):
        clade[i] = direct.get(i, 0) + sum(below(k) for k in tree.kids[i])
        return clade[i]

    for i in tree.order:
        if tree.top(i):
            below(i)
    unknown = sorted(i for i in direct if i not in tree.node)
    return direct, clade, unknown


def rows(tax, ids):
    """-> (ROW_DT array, stats dict) as kslam_kreport_take / kslam_tail_kreport give them"""
    tree = Tree(tax)
    direct, clade, unknown = _counts(tree, ids)
    out = [(i, tree.node[i], direct.get(i, 0), clade[i]) for i in tree.order if clade[i] > 0]
    out += [(i, NO_NODE, direct[i], direct[i]) for i in unknown]
    stats = {"n_ids": sum(direct.values()), "n_unknown_ids": len(unknown), "n_rows": len(out)}
    return np.array(out, dtype=ROW_DT), stats


def text(tax, ids, total):
    """-> the bytes of the report file; ValueError when total is smaller than the ids counted"""
    tree = Tree(tax)
    direct, clade, unknown = _counts(tree, ids)
    counted = sum(direct.values())
    if total < counted:
        raise ValueError("total %d < %d ids" % (total, counted))
    for i in unknown:
        clade[i] = direct[i]
    out = []

    def put(pct_of, own, code, taxid, level, name):
        out.append(b"%s\t%d\t%d\t%s\t%d\t%s%s\n" % (("%6.2f" % (100.0 * pct_of / total)).encode(), pct_of, own, code.encode(), taxid, b"  " * level, name))

    def walk(i, level, letter, number):
        if clade[i] == 0:
            return
        own = LETTER.get(tree.rank[i]) if i in tree.node else None
        letter, number = (own, 0) if own else (letter, number + 1)
        put(clade[i], direct.get(i, 0), letter + (str(number) if number else ""), i, level, tree.name[i] if i in tree.node else b"")
        for k in sorted(tree.kids[i] if i in tree.node else [], key=lambda k: (-clade[k], k)):
            walk(k, level + 1, letter, number)

    if total - counted > 0:
        put(total - counted, total - counted, "U", 0, 0, b"unclassified")
    if counted:
        put(counted, direct.get(1, 0), "R", 1, 0, tree.name[1] if 1 in tree.node else b"root")
        under_root = [i for i in tree.order if tree.top(i) and i != 1] + [i for i in unknown if i != 1]
        for k in sorted(under_root, key=lambda k: (-clade[k], k)):
            walk(k, 1, "R", 0)
    return b"".join(out)


# ---- the worked example of include/kslam_kreport.h (tests/golden/kreport_small.json) ----
SMALL = [(1, 1, "root", "no rank"), (131567, 1, "cellular organisms", "no rank"), (2, 131567, "Bacteria", "superkingdom"),
         (1224, 2, "Proteobacteria", "phylum"), (562, 1224, "Escherichia coli", "species"), (83333, 562, "Escherichia coli K-12", "strain"),
         (10239, 1, "Viruses", "superkingdom"), (10760, 10239, "Escherichia phage T7", "species")]
SMALL_IDS = [562] * 3 + [83333] * 2 + [2, 10760, 999999, 0, 0]

# five nodes, two top-level trees: 10 -> (20 -> 40, 30) and 50
FIVE = [(10, 1, "ten", "phylum"), (20, 10, "twenty", "no rank"), (30, 10, "thirty", "genus"), (40, 20, "forty", "species"), (50, 0, "fifty", "clade")]
CHAIN0, CHAIN_LEN = 1000, 300


def _chain():
    ranks = {0: "superkingdom", 100: "genus", 200: "species"}
    return [(CHAIN0 + k, 1 if k == 0 else CHAIN0 + k - 1, "link%d" % k, ranks.get(k, "no rank")) for k in range(CHAIN_LEN)]


def cases():
    """[{name, tax (bytes), ids (uint32 array)}, ...]: the smallest shapes at which the kernels can go wrong"""
    out = []

    def case(name, records, ids):
        out.append({"name": name, "tax": tax_text(records), "ids": np.asarray(ids, dtype=np.uint32)})

    rng = np.random.default_rng(20)
    pool = np.array([10, 20, 30, 40, 50, 0, 12345], dtype=np.uint32)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1025):          # wave, block and grid edges
        case("n%d" % n, FIVE, rng.choice(pool, n))
    case("all_equal", FIVE, [40] * 1025)                         # one leader per wave
    wide = [(100 + k, 1 if k % 7 == 0 else 100 + k - 1 - (k % 3 if k % 7 > 2 else 0), "w%d" % k, ("species", "genus", "no rank")[k % 3])
            for k in range(1025)]
    case("all_distinct", wide, rng.permutation(np.arange(100, 100 + 1025)))
    case("alternating", FIVE, [20, 30] * 300)                    # two ids lane by lane
    case("runs_across_wave_and_block", FIVE, [10] * 60 + [40] * 11 + [30] * 180 + [40] * 11 + [50] * 120)
    mixed = rng.choice(pool[:5], 700)
    mixed[::7] = 0
    case("zero_in_every_wave", FIVE, mixed)
    case("zeros_only", FIVE, [0] * 300)
    case("table_ends", FIVE, [10, 50, 10, 50, 50])               # the smallest and the largest key
    case("around_every_key", FIVE, [k + d for k in (10, 20, 30, 40, 50) for d in (-1, 0, 1)])
    case("one_node", [(7, 1, "seven", "species")], [7, 7, 7, 6, 8, 0])
    case("no_id_known", [(7, 1, "seven", "species")], [6, 8, 8])
    case("max_id_alone", FIVE, [0xFFFFFFFF])
    far = np.full(500, 10, dtype=np.uint32)
    far[[3, 70, 71, 200, 320, 321, 499]] = 0xFFFFFFFF            # the same unknown id in several waves and blocks
    far[[5, 130, 400]] = 999999
    case("unknown_across_waves", FIVE, far)
    case("unknown_only", FIVE, rng.choice(np.array([9, 0xFFFFFFFF, 999999], dtype=np.uint32), 300))
    chain = _chain()                                             # the up-walk past 64 and 256 levels
    case("chain_leaf", chain, [CHAIN0 + CHAIN_LEN - 1] * 3)
    case("chain_middle", chain, [CHAIN0 + 150] * 2 + [CHAIN0 + 65])
    case("chain_top", chain, [CHAIN0])
    case("chain_all", chain, [CHAIN0 + CHAIN_LEN - 1, CHAIN0 + 257, CHAIN0 + 256, CHAIN0 + 64, CHAIN0 + 63, CHAIN0])
    case("two_trees", FIVE, [40, 50, 50, 30])
    case("repeated_id", FIVE + [(20, 50, "again", "species"), (60, 20, "sixty", "no rank")], [20, 60, 60, 40])   # the first record is kept
    case("undefined_parent", FIVE + [(60, 77, "sixty", "species"), (61, 77, "sixty-one", "no rank")], [60, 61, 61, 77, 10])   # 77: a phantom node
    case("id_one_in_the_tree", SMALL, [1, 1, 562, 0, 10239])
    case("id_one_not_in_the_tree", FIVE, [1, 1, 40])
    case("small", SMALL, SMALL_IDS)
    return out
