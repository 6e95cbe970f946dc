"""The loop of k_apply_s4's walk as the compiler emits it for gfx950 (device-only compile, no GPU needed).

Per cell the walk requests the next cell's inputs (ten loads), computes the current cell and stores its four rows.  Loads and stores
count in vmcnt in order, so a wait for the inputs of the cell about to be computed must leave the ten new loads and the four stores
before them in flight (14), and a wait for anything else in the loop at least the four stores of the cell just computed.  Every
count is the compiler's; it stays exact only while each path through the loop issues the same memory instructions, which is what
this file holds."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources  # noqa: E402

KERNELS = {"hlg": "_ZN4uhdr10k_apply_s4ILi3ELb0EEEvNS_9AppConstsENS_8AppBatchE",
           "pq": "_ZN4uhdr10k_apply_s4ILi2ELb0EEEvNS_9AppConstsENS_8AppBatchE"}
MAX_VALU_PER_TWO_CELLS = 800
PIPED_MIN_VALU = 300   # the pipelined cell is one block of some 360 VALU instructions; nothing else in the loop comes near


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(kernel_resources.HIPCC):
        pytest.skip("hipcc not present")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([kernel_resources.HIPCC] + kernel_resources.FLAGS + ["--cuda-device-only", "-S", os.path.join(kernel_resources.CSRC, "uhdr_kernels.hip"), "-o", out],
                       capture_output=True, text=True, check=True)
        return open(out).read()


class Block:
    def __init__(self, name):
        self.name, self.ins, self.succ = name, [], []

    def ops(self):
        return [s.split()[0] for s in self.ins]

    def valu(self):
        return sum(1 for o in self.ops() if o.startswith("v_"))

    def loads(self):
        return sum(1 for o in self.ops() if o.startswith("global_load"))

    def row_stores(self):
        return sum(1 for o in self.ops() if o == "global_store_dwordx4")

    def other_vmem(self):
        return [o for o in self.ops() if re.match(r"(global_|flat_|buffer_|scratch_)", o) and not o.startswith("global_load") and o != "global_store_dwordx4"]

    def vm_waits(self, after_loads=0, until_store=False):
        """the vmcnt fields of the block's s_waitcnt, optionally only behind its n-th load / in front of its first store"""
        seen, out = 0, []
        for s in self.ins:
            o = s.split()[0]
            if o.startswith("global_load"):
                seen += 1
            elif o.startswith("global_store") and until_store:
                break
            elif o == "s_waitcnt" and seen >= after_loads:
                m = re.search(r"vmcnt\((\d+)\)", s)
                if m:
                    out.append(int(m.group(1)))
        return out


def blocks_of(text, mangled):
    """basic blocks of one kernel: split at labels and behind every branch"""
    lines = text.split("\n")
    start = lines.index(next(l for l in lines if l.startswith(mangled + ":")))
    blocks = [Block("entry")]
    for l in lines[start + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            blocks.append(Block(m.group(1)))
            continue
        s = l.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        blocks[-1].ins.append(s)
        if s.split()[0].startswith("s_cbranch") or s.split()[0] in ("s_branch", "s_endpgm"):
            blocks.append(Block(blocks[-1].name + "+"))
    idx = {b.name: i for i, b in enumerate(blocks)}
    for i, b in enumerate(blocks):
        fall = True
        for s in b.ins:
            o = s.split()[0]
            if o == "s_branch":
                b.succ.append(idx[s.split()[1]])
                fall = False
            elif o.startswith("s_cbranch"):
                b.succ.append(idx[s.split()[1]])
            elif o == "s_endpgm":
                fall = False
        if fall and i + 1 < len(blocks):
            b.succ.append(i + 1)
    return blocks


def components(blocks):
    """strongly connected components with a cycle (Tarjan, iterative)"""
    n = len(blocks)
    index, low, on, stack, out, counter = [None] * n, [0] * n, [False] * n, [], [], 0
    for root in range(n):
        if index[root] is not None:
            continue
        work = [(root, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                index[v] = low[v] = counter
                counter += 1
                stack.append(v)
                on[v] = True
            descended = False
            for j in range(k, len(blocks[v].succ)):
                w = blocks[v].succ[j]
                if index[w] is None:
                    work.append((v, j + 1))
                    work.append((w, 0))
                    descended = True
                    break
                if on[w]:
                    low[v] = min(low[v], index[w])
            if descended:
                continue
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    comp.append(w)
                    if w == v:
                        break
                if len(comp) > 1 or v in blocks[v].succ:
                    out.append(sorted(comp))
            if work:
                p = work[-1][0]
                low[p] = min(low[p], low[v])
    return out


class Walk:
    """the walk's outer loop: its request blocks (ten loads), pipelined cells, the edge form, everything else"""

    def __init__(self, text, mangled):
        self.blocks = blocks_of(text, mangled)
        loops = [c for c in components(self.blocks) if any(self.blocks[i].loads() for i in c) and any(self.blocks[i].row_stores() for i in c)]
        assert len(loops) == 1, "expected one loop with loads and row stores, found %d" % len(loops)
        self.loop = loops[0]
        inl = set(self.loop)
        self.request = [i for i in self.loop if self.blocks[i].loads()]
        self.piped = [i for i in self.loop if self.blocks[i].valu() >= PIPED_MIN_VALU]
        # the edge form: what a request block reaches without passing through a pipelined cell or the other request block
        stop = set(self.request) | set(self.piped)
        self.edge, todo = set(), [w for r in self.request for w in self.blocks[r].succ if w in inl and w not in stop]
        while todo:
            v = todo.pop()
            if v in self.edge:
                continue
            self.edge.add(v)
            todo += [w for w in self.blocks[v].succ if w in inl and w not in stop]
        self.body = [i for i in self.loop if i not in self.edge]   # the two-cell body every interior wave runs

    def describe(self):
        return ["%s valu %d loads %d stores %d waits %s%s" % (self.blocks[i].name, self.blocks[i].valu(), self.blocks[i].loads(), self.blocks[i].row_stores(),
                                                               self.blocks[i].vm_waits(), " (edge form)" if i in self.edge else "") for i in self.loop if self.blocks[i].ins]


@pytest.fixture(scope="module", params=sorted(KERNELS))
def walk(isa, request):
    w = Walk(isa, KERNELS[request.param])
    print("\n".join(w.describe()))
    return w


def test_two_request_groups_of_ten_loads_and_four_row_stores_per_cell(walk):
    assert len(walk.request) == 2 and [walk.blocks[i].loads() for i in walk.request] == [10, 10], walk.describe()
    assert len(walk.piped) == 2 and [walk.blocks[i].row_stores() for i in walk.piped] == [4, 4], walk.describe()
    # the edge form stores its four rows in straight-line code behind its rolled row loop, once per half of the body
    edge_stores = [walk.blocks[i].row_stores() for i in sorted(walk.edge) if walk.blocks[i].row_stores()]
    assert edge_stores == [4, 4], walk.describe()
    inner = [c for c in components([b if i in walk.edge else Block("") for i, b in enumerate(walk.blocks)])]
    assert all(walk.blocks[i].row_stores() == 0 for c in inner for i in c), "a store inside the edge form's rolled loop"
    assert not any(walk.blocks[i].other_vmem() for i in walk.loop), walk.describe()


def test_no_wait_reaches_into_the_stores_of_the_cell_just_computed(walk):
    waits = [(walk.blocks[i].name, n) for i in walk.loop for n in walk.blocks[i].vm_waits()]
    assert waits, "no s_waitcnt vmcnt in the loop at all?"
    assert all(n >= 4 for _, n in waits), waits


def test_waits_behind_a_request_leave_it_and_the_stores_in_flight(walk):
    inl = set(walk.loop)
    for r in walk.request:
        found = list(walk.blocks[r].vm_waits(after_loads=10))
        # ... and in whatever follows, up to the first store of the cell
        seen, todo = set(), [w for w in walk.blocks[r].succ if w in inl]
        while todo:
            v = todo.pop()
            if v in seen or v in walk.request:
                continue
            seen.add(v)
            found += walk.blocks[v].vm_waits(until_store=True)
            if not any(o.startswith("global_store") for o in walk.blocks[v].ops()):
                todo += [w for w in walk.blocks[v].succ if w in inl]
        assert found, "no wait for the current cell's inputs behind %s?" % walk.blocks[r].name
        assert all(n >= 14 for n in found), (walk.blocks[r].name, found)


def test_no_lane_is_masked_outside_the_edge_form(walk):
    masked = [(walk.blocks[i].name, s) for i in walk.body for s in walk.blocks[i].ins if "saveexec" in s.split()[0]]
    assert not masked, masked


def test_two_cell_body_is_within_its_valu_budget(walk):
    n = sum(walk.blocks[i].valu() for i in walk.body)
    print("VALU instructions per two cells: %d" % n)
    assert n <= MAX_VALU_PER_TWO_CELLS, (n, walk.describe())
