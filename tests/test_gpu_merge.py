"""jfgpu_merge_* on the GPU (-m gpu, over capi.Merge): the k-way merge of sorted record bodies in windows of positions
(jellyfish_amd/csrc/kernels_merge.hip.hpp, abi_merge.inl) against a merge written here in Python -- a dict over the inputs'
records, ordered by (pos, key), pos = (M * key) & (size - 1) with M the columns the engine is given (capi.reference_matrix),
applied here through byte tables built with numpy.  The bodies are made here from random keys; output bytes are compared
whole.

Shapes: every key width (k = 8 .. 128, key bytes a multiple of 8 and not), 2 to 17 inputs with counts of 1, 2, 4 and 8
bytes mixed, inputs of no and of one record, overlap from none to total; many keys on one position (size 2^10), dozens of
windows with empty ones among them, one position larger than a window (the buffers grow), the identity matrix; sum, min and
max with and without bounds, sums past the output's maximum, the Jaccard tallies; an unsorted input is refused by name and
the next merge is right."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1


def byte_tables(cols, k):
    """tbl[b, v] = xor of the columns that byte b of a key selects when it has value v (column c-1-j is the image of bit j)."""
    c, kb = 2 * k, (2 * k + 7) // 8
    img = np.zeros(8 * kb, dtype=np.uint64)
    img[:c] = np.asarray(cols, dtype=np.uint64)[::-1]
    tbl = np.zeros((kb, 256), dtype=np.uint64)
    v = np.arange(256)
    for b in range(kb):
        for i in range(8):
            tbl[b] ^= np.where((v >> i) & 1, img[8 * b + i], np.uint64(0)).astype(np.uint64)
    return [[int(x) for x in row] for row in tbl]


class Hash:
    def __init__(self, k, lsize, identity=False):
        from jellyfish_amd import capi
        self.k, self.kb, self.size = k, (2 * k + 7) // 8, 1 << lsize
        self.cols = None if identity else capi.reference_matrix(lsize, 2 * k)
        self.tbl = None if identity else byte_tables(self.cols, k)

    def pos(self, key):
        if self.tbl is None:
            return key & (self.size - 1)
        p = 0
        for b, byte in enumerate(key.to_bytes(self.kb, "little")):
            p ^= self.tbl[b][byte]
        return p & (self.size - 1)


def make_inputs(rng, H, n_per_input, counter_lens, overlap, max_val=None, keep=None):
    """One {key: value} per input.  overlap: the share of an input's keys drawn from a pool all inputs share (the rest are its
    own); keep(pos): only keys on such positions.  Values fill their input's counter width unless max_val caps them."""
    nbits = 2 * H.k

    def draw(n, seen):
        out = []
        while len(out) < n and len(seen) < (1 << nbits):
            x = rng.getrandbits(nbits)
            if x in seen or (keep and not keep(H.pos(x))):
                continue
            seen.add(x)
            out.append(x)
        return out

    seen = set()
    pool = draw(int(max(n_per_input) * overlap), seen)
    inputs = []
    for n, cl in zip(n_per_input, counter_lens):
        shared = rng.sample(pool, min(len(pool), int(n * overlap + 0.5)))
        keys = shared + draw(n - len(shared), seen)
        top = min(max_val or U64, 256 ** cl - 1)
        inputs.append({x: rng.choice([1, 2, 3, top, rng.randrange(1, top + 1)]) for x in keys[:n]})
    return inputs


def bodies_of(H, inputs, counter_lens):
    out = []
    for d, cl in zip(inputs, counter_lens):
        recs = sorted(d.items(), key=lambda kv: (H.pos(kv[0]), kv[0]))
        out.append(np.frombuffer(b"".join(x.to_bytes(H.kb, "little") + v.to_bytes(cl, "little") for x, v in recs), dtype=np.uint8))
    return out


def combine(inputs):
    """{key: (sum mod 2^64, min with 0 for an input that lacks the key, max)}"""
    allk = {}
    for d in inputs:
        for x, v in d.items():
            allk.setdefault(x, []).append(v)
    n = len(inputs)
    return {x: (sum(vs) & U64, min(vs) if len(vs) == n else 0, max(vs)) for x, vs in allk.items()}


def expected_bytes(H, inputs, out_len, op=0, lower=0, upper=U64):
    comb = combine(inputs)
    out = []
    for x in sorted(comb, key=lambda x: (H.pos(x), x)):
        v = comb[x][op]
        if lower <= v <= upper:
            out.append(x.to_bytes(H.kb, "little") + min(v, 256 ** out_len - 1).to_bytes(out_len, "little"))
    return b"".join(out)


def run_merge(gpu, H, bodies, counter_lens, **kw):
    """(output bytes, (windows, records read, records written))"""
    with gpu.Merge(H.k, H.size, H.cols, counter_lens, **kw) as m:
        assert m.out_counter_len == min(counter_lens)
        return m.run(bodies).tobytes(), m.counts()


def check(got, want, orb):
    assert len(got) == len(want), "%d records, expected %d" % (len(got) // orb, len(want) // orb)
    if got != want:
        i = next(i for i in range(0, len(want), orb) if got[i:i + orb] != want[i:i + orb])
        raise AssertionError("record %d: %s, expected %s" % (i // orb, got[i:i + orb].hex(), want[i:i + orb].hex()))


# every word count, key bytes a multiple of 8 and not; the input counts and overlaps go round with it
WIDTHS = [(8, 2, 0.5), (21, 3, 0.3), (32, 5, 1.0), (33, 17, 0.6), (64, 2, 0.0), (65, 3, 0.9), (100, 5, 0.5), (128, 17, 0.2)]


@pytest.mark.parametrize("k,n_inputs,overlap", WIDTHS, ids=["k%d-%dinputs" % (k, n) for k, n, _ in WIDTHS])
def test_merge_sum_every_key_width(gpu, k, n_inputs, overlap):
    rng = random.Random(1000 * k + n_inputs)
    H = Hash(k, min(14, 2 * k - 2))
    cls = [[1, 2, 4, 8][(i + k) % 4] for i in range(n_inputs)]
    ns = [rng.randrange(1500, 2500) if n_inputs <= 5 else rng.randrange(200, 700) for _ in range(n_inputs)]
    if n_inputs >= 5:
        ns[1], ns[3] = 0, 1                                     # an input without records, one with a single record
    inputs = make_inputs(rng, H, ns, cls, overlap)
    assert [len(d) for d in inputs] == ns
    got, counts = run_merge(gpu, H, bodies_of(H, inputs, cls), cls)
    check(got, expected_bytes(H, inputs, min(cls)), H.kb + min(cls))
    assert counts[1] == sum(ns) and counts[2] * (H.kb + min(cls)) == len(got)


def test_many_keys_on_one_position(gpu):
    """size 2^10 and 5,000 records an input: five keys a position on average, so the order inside a position is the keys'."""
    rng = random.Random(7)
    H = Hash(21, 10)
    cls = [4, 2, 4]
    inputs = make_inputs(rng, H, [5000, 4800, 5100], cls, 0.5)
    got, _ = run_merge(gpu, H, bodies_of(H, inputs, cls), cls)
    check(got, expected_bytes(H, inputs, 2), H.kb + 2)


def test_dozens_of_windows_some_empty(gpu):
    """window_records = 256 over 6,000 records whose positions avoid the second quarter and the last eighth of the range."""
    rng = random.Random(8)
    H = Hash(33, 16)
    cls = [4, 4, 8]
    keep = lambda p: not (H.size // 4 <= p < H.size // 2) and p < H.size - H.size // 8
    inputs = make_inputs(rng, H, [2000, 2100, 1900], cls, 0.4, keep=keep)
    held = {H.pos(x) * 24 // H.size for d in inputs for x in d}
    assert len(held) <= 17                                      # of the 24 equal slices the run starts from, 7 or more hold nothing
    got, (windows, n_in, _) = run_merge(gpu, H, bodies_of(H, inputs, cls), cls, window_records=256)
    check(got, expected_bytes(H, inputs, 4), H.kb + 4)
    assert n_in == 6000 and windows >= 24                       # 6000 / 256: no window holds more, so there are at least 24


def test_one_position_larger_than_a_window(gpu):
    """size 2^4 and three inputs of 4,000 records: a position holds about 750 records, three times window_records = 256."""
    rng = random.Random(9)
    H = Hash(21, 4)
    cls = [2, 4, 1]
    inputs = make_inputs(rng, H, [4000, 4000, 4000], cls, 0.5)
    got, counts = run_merge(gpu, H, bodies_of(H, inputs, cls), cls, window_records=256)
    check(got, expected_bytes(H, inputs, 1), H.kb + 1)
    assert counts[0] == 16                                      # a window a position: it cannot be cut further


@pytest.mark.parametrize("k,lsize", [(8, 16), (21, 12)], ids=["k8-size4^k", "k21-low-bits"])
def test_identity_matrix(gpu, k, lsize):
    rng = random.Random(10 + k)
    H = Hash(k, lsize, identity=True)
    cls = [4, 1]
    inputs = make_inputs(rng, H, [3000, 2500], cls, 0.5)
    got, _ = run_merge(gpu, H, bodies_of(H, inputs, cls), cls, window_records=1000)
    check(got, expected_bytes(H, inputs, 1), H.kb + 1)


@pytest.fixture(scope="module")
def op_inputs():
    rng = random.Random(11)
    H = Hash(40, 12)
    cls = [2, 4, 2]
    inputs = make_inputs(rng, H, [1500, 1400, 1600], cls, 0.7, max_val=40)
    return H, cls, inputs, bodies_of(H, inputs, cls)


@pytest.mark.parametrize("op", [0, 1, 2], ids=["sum", "min", "max"])
@pytest.mark.parametrize("lower,upper", [(0, U64), (1, U64), (2, 30), (50, 60), (10 ** 6, U64)],
                         ids=["all", "L1", "L2-U30", "L50-U60", "none"])
def test_operations_and_bounds(gpu, op_inputs, op, lower, upper):
    H, cls, inputs, bodies = op_inputs
    got, _ = run_merge(gpu, H, bodies, cls, op=op, lower=lower, upper=upper, window_records=700)
    want = expected_bytes(H, inputs, 2, op, lower, upper)
    check(got, want, H.kb + 2)
    if lower == 10 ** 6:
        assert len(got) == 0                                    # values of at most 3 * 40: the bounds remove everything
    elif lower == 0 and op != 1:
        assert len(got) // (H.kb + 2) == len(combine(inputs))


@pytest.mark.parametrize("upper", [U64, 300], ids=["unbounded", "U300"])
def test_sums_past_the_output_counter(gpu, upper):
    """One-byte output counts, values up to 200 in three inputs: sums reach 600.  The file holds 255 for them; -U 300 keeps a sum
    of 256 to 300 (as 255) and drops 301, so the filter saw the unclamped value."""
    rng = random.Random(12)
    H = Hash(21, 12)
    cls = [1, 2, 1]
    inputs = make_inputs(rng, H, [1200, 1200, 1200], cls, 1.0, max_val=200)
    sums = [s for s, _, _ in combine(inputs).values()]
    assert any(255 < s <= 300 for s in sums) and any(s > 300 for s in sums)
    got, _ = run_merge(gpu, H, bodies_of(H, inputs, cls), cls, upper=upper)
    want = expected_bytes(H, inputs, 1, 0, 0, upper)
    check(got, want, H.kb + 1)
    assert len(got) // (H.kb + 1) == sum(1 for s in sums if s <= upper)


@pytest.mark.parametrize("k,n_inputs", [(21, 2), (100, 5)])
def test_jaccard_tallies(gpu, k, n_inputs):
    rng = random.Random(13 + k)
    H = Hash(k, 12)
    cls = [[4, 1, 8, 2, 4][i] for i in range(n_inputs)]
    inputs = make_inputs(rng, H, [1500] * n_inputs, cls, 0.8, max_val=1000)
    comb = combine(inputs)
    want = (sum(1 for _, mn, _ in comb.values() if mn > 0), sum(mn for _, mn, _ in comb.values()), len(comb), sum(mx for _, _, mx in comb.values()))
    assert want[0] > 0
    with gpu.Merge(H.k, H.size, H.cols, cls, op=gpu.MERGE_JACCARD, window_records=900) as m:
        assert len(m.run(bodies_of(H, inputs, cls))) == 0       # nothing is written
        assert m.tallies() == want


def test_unsorted_input_is_refused_by_name(gpu):
    """Two neighbouring records of input 1 change places: the call fails and says which input; the same object then merges the
    sorted bodies correctly.  (The kernels read and write in range whatever the order: ranks stay below the window's total.)"""
    rng = random.Random(14)
    H = Hash(21, 12)
    cls = [4, 4, 2]
    inputs = make_inputs(rng, H, [1000, 1100, 900], cls, 0.5)
    good = bodies_of(H, inputs, cls)
    rb = H.kb + 4
    bad = good[1].copy().reshape(-1, rb)
    bad[[600, 601]] = bad[[601, 600]]
    with gpu.Merge(H.k, H.size, H.cols, cls) as m:
        with pytest.raises(gpu.JfgpuError) as e:
            m.run([good[0], bad.reshape(-1), good[2]])
        assert e.value.code == gpu.E_FORMAT and "input 1 " in e.value.msg and "not sorted" in e.value.msg
        check(m.run(good).tobytes(), expected_bytes(H, inputs, 2), H.kb + 2)


def test_too_many_inputs_are_refused_at_create(gpu):
    with pytest.raises(gpu.JfgpuError) as e:
        gpu.Merge(21, 1 << 12, None, [4] * 256)
    assert e.value.code == gpu.E_UNSUPPORTED and "inputs" in e.value.msg
    with gpu.Merge(21, 1 << 12, None, [4] * 64) as m:           # 64 are taken
        assert m.run([np.zeros(0, dtype=np.uint8)] * 64).size == 0
