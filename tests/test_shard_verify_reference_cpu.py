"""CPU: the definitions of tests/shard_verify_reference.py against what the project already trusts -- the oracle's edge hashes
(oracle/twopaco_oracle.c: orc_hash_dump), assemble() of tests/test_gpu_addr_shard.py (the shard layout the end-to-end tests
reassemble filters with) -- and the routing predicates against hand-made wrong answers."""
import os

import numpy as np
import pytest

import shard_verify_reference as R
from helpers import GOLDEN
from oracle import oracle as O

SEED = 20240229
# (fasta, k, L, q): k + 1 > L (the rotation counts of the letters wrap), and a filter wider than 32 bits
TEXTS = [("c2.fa", 29, 22, 5), ("rand6.fa", 9, 33, 5)]


def oracle_of(records, k, L, q):
    o = O.Oracle(k, L, q, O.seed_table(SEED, q, L))
    for r in records:
        o.add_record(r)
    return o


@pytest.fixture(scope="module", params=TEXTS, ids=lambda t: "%s_k%d_L%d" % (t[0][:-3], t[1], t[2]))
def case(request):
    fasta, k, L, q = request.param
    recs = O.read_fasta_records(os.path.join(GOLDEN, fasta))
    o = oracle_of(recs, k, L, q)
    text = o.text.copy()
    assert text.max() <= 4 and text[0] == 4 and text[-1] == 4  # codes, N separators around every record
    yield {"o": o, "recs": recs, "text": text, "k": k, "L": L, "q": q, "table": o.table}
    o.close()


def test_out_edges_equal_the_oracle_at_every_position(case):
    o, text, k, L = case["o"], case["text"], case["k"], case["L"]
    n = 0
    for g in range(text.size - k + 1):
        for c in range(4):
            _, want = o.hash_dump(g, c)
            assert R.edge_hashes(text, g, 4 + c, k, L, case["table"]) == want.tolist(), (g, c)
            n += 1
    assert n > 4 * 5000


def test_in_edges_equal_the_oracle_where_the_text_has_the_letter(case):
    """The in-edge c + T[g .. g+k-1] with c = T[g-1] is the out-edge of g - 1 with the letter T[g+k-1]."""
    o, text, k, L = case["o"], case["text"], case["k"], case["L"]
    n = 0
    for g in range(1, text.size - k + 1):
        c, last = int(text[g - 1]), int(text[g + k - 1])
        if c > 3 or last > 3:
            continue
        _, want = o.hash_dump(g - 1, last)
        assert R.edge_hashes(text, g, c, k, L, case["table"]) == want.tolist(), g
        n += 1
    assert n > 5000


def test_in_edges_of_the_other_letters_equal_an_oracle_on_the_substituted_text(case):
    """For c != T[g-1]: a second oracle on the text with T[g-1] replaced by c, again through the out-edge of g - 1.  One oracle
    serves every position g - 1 = r (mod k + 1) of one shift j (c = T[g-1] + j mod 4): the substituted letters are k + 1 apart, so
    each of these (k+1)-mers holds exactly one of them, its first letter."""
    text, k, L, q = case["text"], case["k"], case["L"], case["q"]
    starts = np.nonzero(text == 4)[0]
    n = 0
    for j in (1, 2, 3):
        for r in range(k + 1):
            sub = text.copy()
            at = np.arange(r, text.size, k + 1)
            at = at[sub[at] < 4]
            sub[at] = (sub[at] + j) % 4
            recs = [np.frombuffer(b"ACGTN", dtype=np.uint8)[sub[a + 1:b]].tobytes() for a, b in zip(starts[:-1], starts[1:])]
            o2 = oracle_of(recs, k, L, q)
            assert (o2.text == sub).all()
            for p in at.tolist():
                g = p + 1
                if g + k > text.size or int(text[g + k - 1]) > 3:
                    continue
                _, want = o2.hash_dump(p, int(text[g + k - 1]))
                assert R.edge_hashes(text, g, int(sub[p]), k, L, case["table"]) == want.tolist(), (g, j)
                n += 1
            o2.close()
    assert n > 3 * 5000


def test_tie_depth_counts_the_equal_leading_functions():
    # functions 0 and 1: letter hashes that no rotation changes and that a letter shares with its complement -- both strands
    # hash alike on every word; function 2 is ordinary
    table = np.array([[0, 31, 31, 0, 0], [31, 0, 0, 31, 0], [1, 2, 4, 11, 0]], dtype=np.uint64)
    text = np.array([4, 0, 1, 2, 3, 0, 0, 4], dtype=np.uint8)
    L, k = 5, 3
    # ACG + T is its own reverse complement: every function ties, the positive strand is taken
    assert R.tie_depth(text, 1, 4 + 3, k, L, table) == 3
    pairs = R.strand_hashes(R.edge_letters(text, 1, 4 + 3, k), L, table)
    assert all(p == n for p, n in pairs) and R.edge_hashes(text, 1, 7, k, L, table) == [p for p, _ in pairs]
    # CGT + A and C + GTA are no palindromes: function 2 decides, the smaller of ITS two values names the strand of every address
    for g, e in ((2, 4 + 0), (3, 1)):
        pairs = R.strand_hashes(R.edge_letters(text, g, e, k), L, table)
        assert R.tie_depth(text, g, e, k, L, table) == 2 and pairs[2][0] != pairs[2][1]
        neg = pairs[2][1] < pairs[2][0]
        assert R.edge_hashes(text, g, e, k, L, table) == [n if neg else p for p, n in pairs]
    assert {R.pick_negative(R.strand_hashes(R.edge_letters(text, g, e, k), L, table)) for g in (1, 2, 3) for e in range(8)} == {False, True}


def _geom(sb, b1, b2, b3):
    mult = 0x9E3779B1
    return {"slice_bits": sb, "b1": b1, "b2": b2, "b3": b3, "perm_mult": mult, "perm_inv": pow(mult, -1, 1 << 32)}


@pytest.mark.parametrize("world", [1, 2, 4, 8])
@pytest.mark.parametrize("geom", [_geom(6, 3, 2, 0), _geom(5, 4, 3, 0), _geom(6, 3, 2, 2), _geom(7, 3, 1, 3)], ids=["2lv_a", "2lv_b", "3lv_a", "3lv_b"])
def test_owner_local_inverts_assemble(geom, world):
    """Scattering a random filter into the ranks' shards by owner_local and reassembling them with assemble() gives it back.
    One rank keeps the filter in its natural layout (csrc/tpc_bins.h: pt_local_addr), which assemble() -- written for the compact
    shards of two ranks and more -- does not describe: there the scatter itself must be the identity."""
    from test_gpu_addr_shard import assemble
    L = geom["slice_bits"] + geom["b1"] + geom["b2"] + geom["b3"]
    rng = np.random.default_rng(L * 8 + world)
    full = rng.integers(0, 1 << 32, ((1 << L) >> 5) + 1, dtype=np.uint64).astype(np.uint32)
    full[-1] = 0
    bits = np.unpackbits(full[:-1].view(np.uint8), bitorder="little")
    A = np.nonzero(bits)[0].astype(np.uint64)
    owner, local = R.owner_local(A, geom, world)
    assert owner.min() >= 0 and owner.max() < world
    shard_bits = (1 << L) // world
    shards = []
    for r in range(world):
        la = local[owner == r].astype(np.int64)
        assert la.size == np.unique(la).size and (la.size == 0 or la.max() < shard_bits)  # injective into the shard
        b = np.zeros(shard_bits, dtype=np.uint8)
        b[la] = 1
        shards.append(np.concatenate([np.packbits(b, bitorder="little").view("<u4").astype(np.uint32), np.zeros(1, dtype=np.uint32)]))
    if world == 1:
        assert (local == A).all() and (shards[0] == full).all()
    else:
        assert (assemble(shards, geom, L, world) == full).all()


def test_chunk_base():
    # 5 tiles on 4 ranks: chunks of 2 tiles, the last rank's chunk is empty and begins at the end of the text
    assert [R.chunk_base(5, r, 4, 2, 0) for r in range(4)] == [0, 2 * 16384, 4 * 16384, 5 * 16384]
    assert R.chunk_base(5, 1, 4, 1, 1) == 3 * 16384
    assert R.chunk_base(7, 0, 1, 3, 2) == 6 * 16384
    assert R.text_tiles(16383) == 1 and R.text_tiles(16384) == 2 and R.text_tiles(5 * 16384 - 1) == 5


def test_sid_parts_round_trip():
    for world in (1, 2, 4, 8, 64):
        lw = world.bit_length() - 1
        for src, rel, e in [(0, 0, 0), (world - 1, (1 << (30 - lw)) - 1, 7), (world // 2, 12345, 4)]:
            sid = R.make_sid(src, rel, e, world)
            assert sid < (1 << 33) and R.sid_parts(sid, world) == (src, rel, e)


# ------------------------------------------------------------------------------------------------ the routing predicates
OWNER = np.array([2, 0, 2, 1, 0, 2], dtype=np.int32)
COUNTS = [2, 1, 3]
PERM = np.array([3, 1, 5, 2, 0, 4], dtype=np.int32)  # owner 0: slots 0-1, owner 1: slot 2, owner 2: slots 3-5


def test_routing_predicates_accept_a_valid_routing():
    assert R.route_violations(PERM, OWNER, COUNTS, 3) == []
    assert R.route_violations(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), [0, 0], 2) == []


def test_routing_predicates_reject_a_duplicate_slot():
    bad = PERM.copy()
    bad[2] = 3  # items 0 and 2, both of owner 2, in slot 3; slot 5 is left empty
    assert not R.route_is_bijection(bad, 6)
    assert R.route_slots_in_ranges(bad, OWNER, COUNTS)  # (each still inside its owner's range: only the bijection sees it)
    assert R.route_violations(bad, OWNER, COUNTS, 3) == ["bijection"]


def test_routing_predicates_reject_a_slot_in_the_neighbours_range():
    bad = PERM.copy()
    bad[3], bad[0] = 3, 2  # the item of owner 1 and an item of owner 2 trade slots: still a bijection
    assert R.route_is_bijection(bad, 6)
    assert not R.route_slots_in_ranges(bad, OWNER, COUNTS)
    assert R.route_violations(bad, OWNER, COUNTS, 3) == ["ranges"]


def test_routing_predicates_reject_a_count_off_by_one():
    assert not R.route_counts_match([2, 2, 2], OWNER, 3)
    assert R.route_violations(PERM, OWNER, [2, 2, 2], 3) == ["counts"]
    assert not R.route_counts_match([2, 1, 3, 0], OWNER, 3)  # one count for every rank, no more
    assert not R.route_is_bijection(PERM[:5], 6) and not R.route_is_bijection(np.array([0, 1, 6, 2, 3, 4]), 6)


def test_all_hit_and_mask_with_bits():
    hit = np.array([1, 1, 0, 1, 1, 1], dtype=np.uint8)
    assert R.all_hit(hit, 3, 2).tolist() == [True, False, True]
    assert R.all_hit(hit, 2, 3).tolist() == [False, True]
    perm = np.array([2, 0, 1, 3, 5, 4])  # survivor 0's answers sit in slots 2 and 0
    assert R.all_hit(hit, 3, 2, perm).tolist() == [False, True, True]
    assert R.all_hit(hit, 0, 4).tolist() == []
    before = np.array([1, 0, 0x80000000], dtype=np.uint32)
    assert R.mask_with_bits(before, [0, 31, 33, 33, 95]).tolist() == [0x80000001, 2, 0x80000000]
    assert before.tolist() == [1, 0, 0x80000000]
