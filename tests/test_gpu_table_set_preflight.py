"""bp_check_table_set on the GPU (csrc/set_check.hip: the keys of a link's ends, the balance in a hash table in HBM, the
scan; csrc/stark_api.cpp: the entry).  The reference is tests/table_set_model.py -- Python integers, a dictionary per
link -- and every comparison is report == model, field for field; the verdict is compared with what
bp_stark_prove_table_set and bp_stark_verify_table_set do with the same set.  CPU side:
tests/test_table_set_preflight.py."""
import numpy as np
import pytest

import air_program_cases as cases
import air_program_port_cases as pc
import table_set_model as model
from air_program_cases import P
from builtin_airs import keccak as KF, keccak_sponge as SP, logic as LG
from proof_protocol_decoder_amd._lib import BpgError
from proof_protocol_decoder_amd.air_program import ALL_ROWS, TRANSITION, Builder
from test_gpu_air_program import constants_cap
from test_gpu_air_program_log_ports import LIMBS, SELF_LINK, count_limbs, range_program, range_witness, self_checked_table
from test_gpu_air_program_ports import LINK, WIDTH, balanced_pair, field, flagged, rows_of
from util import to_dev, to_host

pytestmark = pytest.mark.gpu


def cfg_of(air_id, log_n):
    return cases.cfg_for(air_id, log_n, num_queries=6, pow_bits=6)


def member(bpg, builder, trace, consts=None, air_id=None):
    """a member for the model and for the library: a builder (registered here) or a built-in air_id, its trace (numpy)"""
    reg = air_id if builder is None else bpg.ops.air_register(builder.assemble())
    return {"builder": builder, "air_id": reg, "trace": trace, "consts": consts, "log_n": trace.shape[1].bit_length() - 1}


def arguments(members):
    tables = []
    for m in members:
        t = {"air_id": m["air_id"], "cfg": cfg_of(m["air_id"], m["log_n"]), "trace": to_dev(m["trace"])}
        if m["consts"] is not None:
            t["consts"] = to_dev(m["consts"])
        tables.append(t)
    return tables


def checked(bpg, members, links, want=None):
    """the library's report, compared with the model's field for field"""
    got = bpg.ops.check_table_set(arguments(members), links)
    want = model.report(members, links) if want is None else want
    for k, (g, w) in enumerate(zip(got.links, want)):
        assert g.as_dict() == w, ("link", k, g.as_dict(), w)
    assert len(got.links) == len(want) and got.ok == (all(w["holds"] for w in want) and all(t.ok for t in got.tables))
    assert (got.message == "") == got.ok
    return got, want


def prover_accepts(bpg, members, links):
    """bp_stark_prove_table_set succeeds and bp_stark_verify_table_set accepts its container"""
    tables = arguments(members)
    try:
        container = bpg.ops.stark_prove_table_set(tables, links)
    except BpgError as e:
        assert e.code == -5, e.message
        return False
    statement = [{"air_id": t["air_id"], "cfg": t["cfg"]} for t in tables]
    caps = [None if m["consts"] is None else constants_cap(bpg, to_dev(m["consts"]), m["log_n"]) for m in members]
    try:
        bpg.ops.stark_verify_table_set(statement, links, container, const_caps=caps)
    except BpgError as e:
        assert e.code == -5, e.message
        return False
    return True


# ---------------------------------------------------------------------------------------------- the sets


def flag_pair(bpg):
    a, b, a_rows, b_rows = balanced_pair()
    fp = pc.flag_program()
    return [member(bpg, fp, a), member(bpg, fp, b)], a_rows, b_rows


def three_flag_tables(bpg):
    """two looking tables (2^5, 2^6) into one looked port (2^7): test_two_looking_ports_on_two_tables_into_one_looked_port's"""
    rng = np.random.default_rng(0xD200)
    s1 = [[int(v) for v in field(rng, WIDTH)] for _ in range(6)]
    s2 = [[int(v) for v in field(rng, WIDTH)] for _ in range(11)] + [list(s1[0])]
    exposed = [(s1 + s2)[k] for k in rng.permutation(18)]
    traces = [flagged(5, rows_of(5, rng, 6), s1, rng), flagged(6, rows_of(6, rng, 12), s2, rng), flagged(7, rows_of(7, rng, 18), exposed, rng)]
    fp = pc.flag_program()
    return [member(bpg, fp, t) for t in traces], [([(0, 0), (1, 0)], (2, 0))]


def self_range_table(bpg, limb_kind_multiplicity=False):
    _, t, consts, _ = self_checked_table(bpg, limb_kind_multiplicity)
    return [member(bpg, range_program(limb_kind_multiplicity), t, consts)], SELF_LINK


def looked_range_program():
    b = Builder(8, n_const=1)
    count = b.family(1, TRANSITION, 1)
    b.unit()
    b.emit(count, b.nxt(5) - b.loc(5) - 1)
    b.log_port(b.loc(4), [b.cst(0)], multiplicity=True)
    return b


def two_looking_range_tables(bpg):
    """2^5 and 2^7 rows of two 8-bit limbs each into a 2^8-row table: test_two_looking_tables_into_one_range_table's"""
    rng = np.random.default_rng(0x1D100)
    a, c = range_witness(5, 256, rng, n_limbs=2), range_witness(7, 256, rng, n_limbs=2)
    mult = count_limbs(bpg, a, 8, n_limbs=2)
    count_limbs(bpg, c, 8, out=mult, n_limbs=2)
    table = np.zeros((8, 256), dtype=np.uint64)
    table[4], table[5] = to_host(mult), np.arange(256, dtype=np.uint64)
    looking = range_program(n_limbs=2, looked=False)
    members = [member(bpg, looking, a), member(bpg, looking, c),
               member(bpg, looked_range_program(), table, np.arange(256, dtype=np.uint64).reshape(1, 256))]
    return members, [([(0, 0), (0, 1), (1, 0), (1, 1)], (2, 0))]


def memory_reader(bpg):
    """a run-time table looking words up in the built-in memory table (AIR 3)"""
    from builtin_airs import memory
    log = memory.random_log(64, 0xE000, n_addr=6)
    rng = np.random.default_rng(0xE001)
    asked = rows_of(6, rng, 9)
    mem = bpg.ops.memory_trace(6, inputs=to_dev(log))
    mem[pc.MEM_G, asked] = 1
    words = [[int(v) for v in log[row]] for row in asked]
    r = flagged(5, rows_of(5, rng, 9), [words[k] for k in rng.permutation(9)], rng, width=11, n_cols=16)
    return [member(bpg, pc.flag_program(width=11, n_cols=16), r), member(bpg, None, to_host(mem), air_id=3)], LINK


# ---------------------------------------------------------------------------------------------- 1. balanced sets


@pytest.mark.parametrize("case", ["pair", "three-tables", "self-range", "two-looking-range", "memory"])
def test_balanced_sets_agree_with_the_prover(bpg, case):
    members, links = {"pair": lambda: (flag_pair(bpg)[0], LINK), "three-tables": lambda: three_flag_tables(bpg),
                      "self-range": lambda: self_range_table(bpg), "two-looking-range": lambda: two_looking_range_tables(bpg),
                      "memory": lambda: memory_reader(bpg)}[case]()
    got, want = checked(bpg, members, links)
    assert got.ok and all(w["holds"] and w["n_looking"] > 0 and w["n_looked"] > 0 for w in want)
    assert got.links[0].is_log == (case in ("self-range", "two-looking-range"))
    assert prover_accepts(bpg, members, links)


# ---------------------------------------------------------------------------------------------- 2. unbalanced sets


@pytest.mark.parametrize("case", ["cell", "stranger", "unflagged"])
def test_unbalanced_sets_are_named(bpg, case):
    """test_a_set_that_does_not_balance_is_refused_by_the_prover_and_the_verifier's three cases"""
    members, a_rows, b_rows = flag_pair(bpg)
    a, b = members[0]["trace"], members[1]["trace"]
    if case == "cell":          # one tuple cell changed on a flagged row of A
        a[2, a_rows[4]] = (int(a[2, a_rows[4]]) + 1) % P
    elif case == "stranger":    # the tuple sent twice is exposed once, next to a stranger
        twice = [r for r in b_rows if [int(v) for v in b[1:1 + WIDTH, r]] == [int(v) for v in a[1:1 + WIDTH, a_rows[3]]]]
        assert len(twice) == 2
        b[1, twice[1]] = (int(b[1, twice[1]]) + 12345) % P
    else:                       # a flagged row of B unflagged
        b[0, b_rows[7]] = 0
    got, (want,) = checked(bpg, members, LINK)
    link = got.links[0]
    assert not got.ok and all(t.ok for t in got.tables) and not link.holds
    assert "link 0" in got.message and "looking row %d " % want["first_looking_row"] in got.message \
        and "looked row %d " % want["first_looked_row"] in got.message and "port 0 of table 0" in got.message \
        and "port 0 of table 1" in got.message, got.message
    assert link.n_unbalanced == want["n_unbalanced"] == {"cell": 2, "stranger": 2, "unflagged": 1}[case]
    assert (link.first_looking_end, link.first_looking_row, link.first_looked_row) == \
        (want["first_looking_end"], want["first_looking_row"], want["first_looked_row"])
    if case == "cell":
        assert link.first_looking_row == a_rows[4]
    if case == "stranger":      # sent twice, exposed once: that value is off by one, and the stranger by one
        assert link.first_looking_row == min(a_rows[3], a_rows[9]) and link.first_looked_row == twice[0] < twice[1]
    if case == "unflagged":
        assert link.n_looked == 9 and link.n_looking == 10
    with pytest.raises(BpgError) as e:
        bpg.ops.stark_prove_table_set(arguments(members), LINK)
    assert e.value.code == -5 and "link 0 does not hold" in e.value.message


# ---------------------------------------------------------------------------------------------- 3. log links


def test_a_limb_out_of_range_names_the_looking_row(bpg):
    """test_a_limb_out_of_range_is_refused_by_the_prover_and_the_verifier's witness"""
    members, links = self_range_table(bpg)
    t = members[0]["trace"]
    row = int(np.nonzero(t[3])[0][5])
    t[1, row] = 64
    rest = t[3].copy()
    rest[row] = 0
    mult = bpg.ops.range_multiplicities(to_dev(t)[[0, 2]], 6, filter=to_dev(t[3]))
    t[4] = to_host(bpg.ops.range_multiplicities(to_dev(t)[1:2], 6, filter=to_dev(rest), out=mult))
    got, (want,) = checked(bpg, members, links)
    link = got.links[0]
    assert not got.ok and link.is_log and link.n_unbalanced == 1
    assert (link.first_looking_end, link.first_looking_row, link.first_looked_row) == (1, row, -1)
    assert "link 0" in got.message and "looking row %d (port 1 of table 0)" % row in got.message, got.message
    assert not prover_accepts(bpg, members, links)


def test_a_multiplicity_off_by_one_names_the_values_row(bpg):
    members, links = self_range_table(bpg)
    t = members[0]["trace"]
    value = int(t[0, int(np.nonzero(t[3])[0][0])])
    t[4, value] += np.uint64(1)
    got, (want,) = checked(bpg, members, links)
    link = got.links[0]
    carrying = sorted((k, int(r)) for k in range(LIMBS) for r in np.nonzero((t[k] == value) & (t[3] == 1))[0])
    assert not got.ok and link.n_unbalanced == 1 and link.first_looked_row == value      # the constant column holds v at row v
    assert (link.first_looking_end, link.first_looking_row) == carrying[0]
    assert not prover_accepts(bpg, members, links)


@pytest.mark.parametrize("limb_kind_multiplicity", [False, True], ids=["kind-1", "kind-2"])
def test_filters_that_cancel_on_a_stranger_are_a_bad_filter_only_where_a_bit_is_demanded(bpg, limb_kind_multiplicity):
    """test_the_bit_constraint_is_what_makes_membership_sound's witness: the limb 64 sent with filters 1 and p - 1"""
    members, links = self_range_table(bpg, limb_kind_multiplicity)
    t = members[0]["trace"]
    r1, r2 = (int(v) for v in np.nonzero(t[3] == 0)[0][:2])
    t[:LIMBS, r1] = t[:LIMBS, r2] = 64
    t[3, r1], t[3, r2] = 1, P - 1
    got, (want,) = checked(bpg, members, links)
    link = got.links[0]
    assert link.n_unbalanced == 0 and got.tables[0].ok
    if limb_kind_multiplicity:
        assert got.ok and link.holds and link.bad_filter_end == -1
    else:
        assert not got.ok and not link.holds
        assert (link.bad_filter_end, link.bad_filter_row, link.bad_filter_value) == (0, r2, P - 1)
        assert "link 0" in got.message and "port 0 of table 0" in got.message and "row %d" % r2 in got.message \
            and str(P - 1) in got.message, got.message
    assert prover_accepts(bpg, members, links) == limb_kind_multiplicity


# ---------------------------------------------------------------------------------------------- 4. a non-bit product filter


def loose_program():
    """test_a_filter_that_is_no_bit_is_rejected_at_zeta's: the flag column has no constraint of its own"""
    b = Builder(8)
    count = b.family(1, TRANSITION, 1)
    b.unit()
    b.emit(count, b.nxt(4) - b.loc(4) - 1)
    b.port(b.loc(0), [b.loc(1 + j) for j in range(WIDTH)])
    return b


def test_a_filter_that_is_no_bit_on_a_product_port_is_named_with_its_value(bpg):
    a, b, a_rows, _ = balanced_pair()
    a[0, a_rows[2]] = 2
    members = [member(bpg, loose_program(), a), member(bpg, pc.flag_program(), b)]
    assert bpg.ops.check_air_trace(members[0]["air_id"], to_dev(a)).ok        # the checker drops the ports: the gap this closes
    got, (want,) = checked(bpg, members, LINK)
    link = got.links[0]
    assert not got.ok and got.tables[0].ok and got.tables[1].ok
    assert (link.bad_filter_end, link.bad_filter_row, link.bad_filter_value) == (0, a_rows[2], 2)
    assert link.n_unbalanced == 1 and link.first_looking_row == a_rows[2]     # the row enters the balance with its 2
    assert "link 0" in got.message and "no bit" in got.message and "row %d" % a_rows[2] in got.message and "it is 2" in got.message
    assert not prover_accepts(bpg, members, LINK)


# ---------------------------------------------------------------------------------------------- 5. a member's own AIR


def test_a_member_that_breaks_its_own_air_is_named_and_the_links_are_still_reported(bpg):
    members, links = three_flag_tables(bpg)
    t = members[1]["trace"]
    t[WIDTH + 1, 40] = (int(t[WIDTH + 1, 40]) + 7) % P                        # the counter: transitions 39 -> 40 -> 41
    got, want = checked(bpg, members, links)
    alone = bpg.ops.check_air_trace(members[1]["air_id"], to_dev(t), max_rows=8, max_viol=8)
    assert not got.ok and got.links[0].holds and got.tables[0].ok and got.tables[2].ok
    assert got.tables[1].n_violated_rows == alone.n_violated_rows == 2 and got.tables[1].rows == alone.rows == [39, 40]
    key = lambda v: (v.row, v.constraint, v.family, v.kind, v.value)
    assert [key(v) for v in got.tables[1].violations] == [key(v) for v in alone.violations] and len(alone.violations) == 2
    assert "table 1 " in got.message and "row 39 violates constraint 1 " in got.message and "2 rows in all" in got.message, got.message
    assert not prover_accepts(bpg, members, links)


# ---------------------------------------------------------------------------------------------- 6. shapes


@pytest.mark.parametrize("log_n", [5, 6, 8, 9], ids=["half-a-wave", "one-wave", "one-workgroup", "two-workgroups"])
def test_flag_tables_of_the_sizes_the_launch_changes_at(bpg, log_n):
    """both ends 2^log_n rows, three quarters of them active, the last row among them; then one cell changed"""
    n = 1 << log_n
    rng = np.random.default_rng(0x6100 + log_n)
    k = 3 * n // 4
    sent = [[int(v) for v in field(rng, WIDTH)] for _ in range(k)]
    a_rows = sorted(int(v) for v in rng.choice(n - 1, size=k - 1, replace=False)) + [n - 1]
    b_rows = rows_of(log_n, rng, k)
    fp = pc.flag_program()
    members = [member(bpg, fp, flagged(log_n, a_rows, sent, rng)), member(bpg, fp, flagged(log_n, b_rows, [sent[j] for j in rng.permutation(k)], rng))]
    got, (want,) = checked(bpg, members, LINK)
    assert got.ok and want["n_looking"] == want["n_looked"] == k
    members[0]["trace"][1, n - 1] = (int(members[0]["trace"][1, n - 1]) + 1) % P
    got, (want,) = checked(bpg, members, LINK)
    assert got.links[0].n_unbalanced == 2 and got.links[0].first_looking_row == n - 1


def eight_limb_program():
    """eight kind-1 ports, one limb column each, one filter column"""
    b = Builder(16)
    count = b.family(1, TRANSITION, 1)
    b.unit()
    b.emit(count, b.nxt(9) - b.loc(9) - 1)
    for k in range(8):
        b.log_port(b.loc(8), [b.loc(k)])
    return b


def test_eight_ports_of_equal_limbs_the_contention_worst_case(bpg):
    n = 1 << 12
    a = np.zeros((16, n), dtype=np.uint64)
    a[:8], a[8], a[9] = 7, 1, np.arange(n, dtype=np.uint64)
    table = np.zeros((8, 32), dtype=np.uint64)
    table[4, 7], table[5] = 8 * n, np.arange(32, dtype=np.uint64)
    members = [member(bpg, eight_limb_program(), a), member(bpg, looked_range_program(), table, np.arange(32, dtype=np.uint64).reshape(1, 32))]
    links = [([(0, k) for k in range(8)], (1, 0))]
    got, (want,) = checked(bpg, members, links)
    assert got.ok and (want["n_looking"], want["n_looked"]) == (8 * n, 1)
    table[4, 7] -= np.uint64(1)
    got, (want,) = checked(bpg, members, links)
    link = got.links[0]
    assert link.n_unbalanced == 1 and (link.first_looking_end, link.first_looking_row, link.first_looked_row) == (0, 0, 7)


def test_thousands_of_distinct_tuples_exposed_in_a_permutation(bpg):
    """2^14 rows, every row active, pairwise distinct 3-element tuples: 2^14 occupied slots of 2^16, long probe runs"""
    n = 1 << 14
    rng = np.random.default_rng(0x6300)
    i = np.arange(n, dtype=np.uint64)
    a = np.zeros((8, n), dtype=np.uint64)
    a[0], a[1], a[2], a[3], a[4] = 1, i, i * i + np.uint64(1), np.uint64(7) * i, i + np.uint64(5)
    b = a.copy()
    b[1:4] = a[1:4][:, rng.permutation(n)]
    fp = pc.flag_program()
    members = [member(bpg, fp, a), member(bpg, fp, b)]
    ends = [model.member_ports(m)[0][0] for m in members]                    # evaluated once for both halves
    got, _ = checked(bpg, members, LINK, want=[model.link_report(ends, [True, True], False)])
    assert got.ok and got.links[0].n_looking == got.links[0].n_looked == n
    row = 9001
    b[2, row] = (int(b[2, row]) + 1) % P
    f, t = ends[1][row]
    ends[1][row] = (f, [t[0], int(b[2, row]), t[2]])
    got, (want,) = checked(bpg, members, LINK, want=[model.link_report(ends, [True, True], False)])
    assert got.links[0].n_unbalanced == 2 and got.links[0].first_looked_row == row
    assert int(a[1, got.links[0].first_looking_row]) == t[0]


def test_a_link_whose_active_rows_number_a_power_of_two(bpg):
    """every row of both 2^5-row ends active: 2^6 active rows"""
    rng = np.random.default_rng(0x6400)
    sent = [[int(v) for v in field(rng, WIDTH)] for _ in range(32)]
    fp = pc.flag_program()
    members = [member(bpg, fp, flagged(5, range(32), sent, rng)), member(bpg, fp, flagged(5, range(32), [sent[j] for j in rng.permutation(32)], rng))]
    got, (want,) = checked(bpg, members, LINK)
    assert got.ok and want["n_looking"] + want["n_looked"] == 64


def test_ends_of_different_tuple_lengths(bpg):
    """(a, b) against (a, b, 0): one value to the proof, and to the pre-flight"""
    rng = np.random.default_rng(0x6500)
    sent = [[int(v) for v in field(rng, 2)] for _ in range(7)]
    a = flagged(5, rows_of(5, rng, 7), sent, rng, width=2)
    b = flagged(6, rows_of(6, rng, 7), [sent[j] + [0] for j in rng.permutation(7)], rng, width=3)
    members = [member(bpg, pc.flag_program(width=2), a), member(bpg, pc.flag_program(width=3), b)]
    got, _ = checked(bpg, members, LINK)
    assert got.ok and prover_accepts(bpg, members, LINK)


def two_ended_program():
    """port 0: filter column 0, tuple columns 1, 2; port 1: filter column 3, tuple columns 4, 5; column 6 counts"""
    b = Builder(8)
    bit = b.family(2, ALL_ROWS, 2)
    count = b.family(1, TRANSITION, 1)
    b.unit()
    b.emit(bit, b.loc(0) * b.loc(0) - b.loc(0))
    b.emit(bit + 1, b.loc(3) * b.loc(3) - b.loc(3))
    b.emit(count, b.nxt(6) - b.loc(6) - 1)
    b.port(b.loc(0), [b.loc(1), b.loc(2)])
    b.port(b.loc(3), [b.loc(4), b.loc(5)])
    return b


def test_a_link_with_both_ends_in_one_table(bpg):
    rng = np.random.default_rng(0x6600)
    n = 64
    t = np.zeros((8, n), dtype=np.uint64)
    t[[1, 2, 4, 5]] = field(rng, (4, n))
    t[6] = np.arange(n, dtype=np.uint64)
    out_rows, in_rows = rows_of(6, rng, 11), rows_of(6, rng, 11)
    t[0, out_rows], t[3, in_rows] = 1, 1
    for r_in, r_out in zip(in_rows, [out_rows[j] for j in rng.permutation(11)]):
        t[4:6, r_in] = t[1:3, r_out]
    members, links = [member(bpg, two_ended_program(), t)], [([(0, 0)], (0, 1))]
    got, _ = checked(bpg, members, links)
    assert got.ok and prover_accepts(bpg, members, links)
    t[4, in_rows[3]] = (int(t[4, in_rows[3]]) + 1) % P
    got, (want,) = checked(bpg, members, links)
    assert got.links[0].n_unbalanced == 2 and got.links[0].first_looked_row == in_rows[3]


def test_eight_looking_ports_and_an_unbalanced_value_on_a_later_end(bpg):
    """port k of flag_program(ports=8) sends the tuple shifted by k; the looked table exposes all eight shifts; the copy
    of shift 3 of one row is changed: the first unmatched looking row is on end 3"""
    rng = np.random.default_rng(0x6700)
    sent = [[int(v) for v in field(rng, WIDTH)] for _ in range(5)]
    a_rows = rows_of(5, rng, 5)
    a = flagged(5, a_rows, sent, rng)
    exposed = [[(v + k) % P for v in s] for k in range(8) for s in sent]
    b_rows = rows_of(6, rng, 40)
    order = [int(j) for j in rng.permutation(40)]
    b = flagged(6, b_rows, [exposed[j] for j in order], rng)
    members = [member(bpg, pc.flag_program(ports=8), a), member(bpg, pc.flag_program(), b)]
    links = [([(0, k) for k in range(8)], (1, 0))]
    got, _ = checked(bpg, members, links)
    assert got.ok
    where = b_rows[order.index(3 * 5 + 2)]                                  # shift 3 of sent[2]
    b[3, where] = (int(b[3, where]) + 1) % P
    got, (want,) = checked(bpg, members, links)
    link = got.links[0]
    assert (link.n_unbalanced, link.first_looking_end, link.first_looking_row, link.first_looked_row) == (2, 3, a_rows[2], where)
    assert "port 3 of table 0" in got.message


def test_two_built_in_members_are_read_as_the_header_lists_them(bpg):
    """byte packing (AIR 5) looking into memory (AIR 3), both from seeds: the memory table exposes every third row and,
    written over four of them, the words of the first four packing rows -- those balance, nothing else does (and the
    overwritten memory table breaks its own AIR, which is table 1's report, not the link's)"""
    pack, mem = to_host(bpg.ops.byte_packing_trace(5, seed=3)), to_host(bpg.ops.memory_trace(6, seed=4))
    mem[model.MEM_G, ::3] = 1
    sending = [i for i in range(32) if int(pack[model.PACK_LEN:model.PACK_LEN + 32, i].sum()) != 0]
    assert len(sending) >= 4
    for i, row in zip(sending[:4], (0, 3, 6, 9)):
        mem[0, row], mem[1, row], mem[2, row] = pack[0, i], pack[model.PACK_ADDR, i], pack[model.PACK_TS, i]
        mem[3:11, row] = pack[model.PACK_VAL:model.PACK_VAL + 8, i]
    members = [member(bpg, None, pack, air_id=5), member(bpg, None, mem, air_id=3)]
    got, (want,) = checked(bpg, members, LINK)
    assert not got.ok and got.tables[0].ok and not got.tables[1].ok and "table 1 " in got.message
    assert want["n_looking"] == len(sending) and want["n_looked"] == 22 and want["n_unbalanced"] >= len(sending) - 4
    assert got.links[0].first_looking_row == sending[4] and got.links[0].first_looked_row == 12 and got.links[0].bad_filter_end == -1


# the three tables a transaction's sponge ties together, as a set: every port of the sponge table (AIR 6) is in a link
SPONGE_LINKS = [([(0, 0)], (1, 0)), ([(0, 1 + m) for m in range(5)], (2, 0))]


def sponge_keccak_logic(bpg):
    """seeded 2^5-row tables of AIRs 6, 1 and 2 on the host (the seeded looked tables expose nothing: their g is zero), and
    the sponge rows that send"""
    sponge, keccak, logic = (to_host(bpg.ops.air_trace(a, 5, seed=s)) for a, s in ((6, 3), (1, 4), (2, 5)))
    assert not keccak[KF.COL_FILTER].any() and not logic[LG.COL_FILTER].any()
    sending = [i for i in range(32) if int(sponge[SP.COL_FULL, i]) + int(sponge[SP.COL_FINAL, i])]
    assert len(sending) >= 5
    return sponge, keccak, logic, sending


def test_the_sponge_and_keccak_f_tables_are_read_as_the_header_lists_them(bpg):
    """sponge port 0 (AIR 6) looking into Keccak-f (AIR 1): 2^5 rows hold one whole permutation, rows 0 .. 23; the tuple of
    one sponge row is written over its input limbs (row 0, read 23 rows up) and its output limbs (row 23), with g set on
    row 23 -- that row balances, every other sending sponge row does not.  (The overwritten Keccak-f table breaks its own
    AIR: table 1's report.)"""
    sponge, keccak, logic, sending = sponge_keccak_logic(bpg)
    r = sending[1]
    _, tup = model.builtin_ports(6, sponge[:, r:r + 1])[0][0]
    keccak[KF.COL_A:KF.COL_A + 50, 0] = tup[:50]
    keccak[KF.COL_APPP:KF.COL_APPP + 2, 23], keccak[KF.COL_APP + 2:KF.COL_APP + 50, 23] = tup[50:52], tup[52:]
    keccak[KF.COL_FILTER, 23] = 1
    members = [member(bpg, None, sponge, air_id=6), member(bpg, None, keccak, air_id=1), member(bpg, None, logic, air_id=2)]
    got, want = checked(bpg, members, SPONGE_LINKS)
    assert not got.ok and got.tables[0].ok and not got.tables[1].ok
    assert want[0]["n_looking"] == len(sending) and want[0]["n_looked"] == 1 and 1 <= want[0]["n_unbalanced"] <= len(sending) - 1
    assert got.links[0].first_looking_row == sending[0] and got.links[0].first_looked_row == -1
    assert want[1]["n_looking"] == 5 * len(sending) and want[1]["n_looked"] == 0


def test_the_sponge_and_logic_tables_are_read_as_the_header_lists_them(bpg):
    """sponge ports 1 .. 5 (AIR 6) looking into logic (AIR 2): the five XORs of the first four sending sponge rows are
    written over logic rows 0 .. 19 (row 5k + m: limb group m of the k-th of them), then one result limb of logic row 0 is
    flipped: limb group 0 of the first sending row.  Those twenty tuples less one balance, nothing else does, and the
    first unmatched looking row is that row at end 0, the flipped limb's group.  The end alone does not show that the flip
    was seen -- the uncovered rows are unmatched at end 0 too, and a flip in another group would hide behind them: the
    smallest (end, row) is at end 0 either way -- the ROW does (without the flip it is the fifth sending row, the looked
    row 2), and so does the comparison with the model, field for field."""
    sponge, keccak, logic, sending = sponge_keccak_logic(bpg)
    ports = model.builtin_ports(6, sponge)
    for k, i in enumerate(sending[:4]):
        for m in range(5):
            _, tup = ports[1 + m][i]
            row = 5 * k + m
            logic[LG.COL_OP:LG.COL_OP + 3, row] = tup[:3]
            for j in range(8):
                logic[LG.COL_IN0 + 32 * j:LG.COL_IN0 + 32 * j + 32, row] = [(tup[3 + j] >> z) & 1 for z in range(32)]
                logic[LG.COL_IN1 + 32 * j:LG.COL_IN1 + 32 * j + 32, row] = [(tup[11 + j] >> z) & 1 for z in range(32)]
            logic[LG.COL_RES:LG.COL_RES + 8, row] = tup[19:]
            logic[LG.COL_FILTER, row] = 1
    logic[LG.COL_RES + 1, 0] ^= np.uint64(0x40)
    members = [member(bpg, None, sponge, air_id=6), member(bpg, None, keccak, air_id=1), member(bpg, None, logic, air_id=2)]
    got, want = checked(bpg, members, SPONGE_LINKS)
    assert not got.ok and got.tables[0].ok
    assert want[1]["n_looking"] == 5 * len(sending) and want[1]["n_looked"] == 20
    assert 2 <= want[1]["n_unbalanced"] <= 5 * len(sending) - 19 + 1      # at most: every uncovered tuple, the flipped one on both sides
    lk = got.links[1]
    assert (lk.first_looking_end, lk.first_looking_row, lk.first_looked_row) == (0, sending[0], 0) and lk.bad_filter_end == -1


# ---------------------------------------------------------------------------------------------- 7. seeded differential run

GROUP = 4   # columns per port of a random table: filter, two tuple elements, one spare


def random_table_program(kinds):
    """one port per entry of `kinds` (0 product, 1 log bit, 2 log multiplicity), port l over columns 4l .. 4l + 2; the
    table's own constraint is a counter in column 4 * len(kinds): no filter is constrained by the table itself"""
    n_cols = max(8, GROUP * len(kinds) + 1)
    b = Builder(n_cols)
    count = b.family(1, TRANSITION, 1)
    b.unit()
    c = GROUP * len(kinds)
    b.emit(count, b.nxt(c) - b.loc(c) - 1)
    for l, kind in enumerate(kinds):
        f, t = b.loc(GROUP * l), [b.loc(GROUP * l + 1), b.loc(GROUP * l + 2)]
        if kind == 0:
            b.port(f, t)
        else:
            b.log_port(f, t, multiplicity=kind == 2)
    return b


def random_set(bpg, seed):
    """1 .. 3 tables of 2^5 .. 2^8 rows, 1 .. 4 links of all three port kinds, tuples from {0, 1, 2}^2 so that
    duplicates and partial cancellations abound; balanced by construction, then 0 .. 3 perturbations -- a cell, a flag,
    a multiplicity, a filter set to 2.  No table constrains a filter of its own, so apart from what a perturbation does
    to a port every member satisfies its AIR."""
    rng = np.random.default_rng(seed)
    n_tables = int(rng.integers(1, 4))
    log_ns = [int(rng.integers(5, 9)) for _ in range(n_tables)]
    kinds = [[] for _ in range(n_tables)]          # per table the kinds of its ports
    links, ends_of = [], []                        # ends_of[k] = [(table, port, kind, looked)]
    for _ in range(int(rng.integers(1, 5))):
        log = bool(rng.integers(0, 2))
        ends = []
        for m in range(int(rng.integers(1, 3)) + 1):
            looked = m == 0
            table = int(rng.integers(0, n_tables))
            if len(kinds[table]) == 8:
                table = min(range(n_tables), key=lambda t: len(kinds[t]))
            if len(kinds[table]) == 8:
                continue
            kind = 0 if not log else (2 if looked and rng.integers(0, 4) else int(rng.integers(1, 3)))
            kinds[table].append(kind)
            ends.append((table, len(kinds[table]) - 1, kind, looked))
        if len(ends) < 2 or not ends[0][3]:
            for table, _, _, _ in reversed(ends):
                kinds[table].pop()
            continue
        links.append(([(t, p) for t, p, _, looked in ends if not looked], [(t, p) for t, p, _, looked in ends if looked][0]))
        ends_of.append(ends)
    # a table without a port cannot be a member: give it a self-link of two product ports
    for t in range(n_tables):
        if not kinds[t]:
            kinds[t] += [0, 0]
            links.append(([(t, 0)], (t, 1)))
            ends_of.append([(t, 1, 0, True), (t, 0, 0, False)])
    traces = []
    for t in range(n_tables):
        n = 1 << log_ns[t]
        tr = np.zeros((max(8, GROUP * len(kinds[t]) + 1), n), dtype=np.uint64)
        for l in range(len(kinds[t])):
            tr[GROUP * l + 1:GROUP * l + 3] = rng.integers(0, 3, size=(2, n), dtype=np.uint64)   # unflagged noise
        tr[GROUP * len(kinds[t])] = np.arange(3, 3 + n, dtype=np.uint64)
        traces.append(tr)
    active = []                                    # (table, port, kind, row) of every row that carries something
    for ends in ends_of:
        looking = [e for e in ends if not e[3]]
        (lt, lp, lkind, _), = [e for e in ends if e[3]]
        free = {(t, p): [int(r) for r in rng.permutation(1 << log_ns[t])] for t, p, _, _ in ends}
        demand = {}
        for t, p, kind, _ in looking:
            for _ in range(int(rng.integers(1, 6))):     # at most 2 ends x 5 sends x 3: the looked rows fit 2^5
                v = tuple(int(x) for x in rng.integers(0, 3, size=2))
                f = int(rng.integers(1, 4)) if kind == 2 else 1
                row = free[(t, p)].pop()
                traces[t][GROUP * p:GROUP * p + 3, row] = [f, v[0], v[1]]
                demand[v] = demand.get(v, 0) + f
                active.append((t, p, kind, row))
        for v, total in demand.items():
            parts = [total] if lkind == 2 and rng.integers(0, 2) else ([1] * total if lkind != 2 else [1, total - 1] if total > 1 else [1])
            for f in parts:
                row = free[(lt, lp)].pop()
                traces[lt][GROUP * lp:GROUP * lp + 3, row] = [f, v[0], v[1]]
                active.append((lt, lp, lkind, row))
    for _ in range(int(rng.choice([0, 0, 0, 1, 1, 2, 3]))):     # (nearly half of the sets stay balanced)
        t, p, kind, row = active[int(rng.integers(0, len(active)))]
        what = int(rng.integers(0, 4))
        c = GROUP * p
        if what == 0:                               # a cell
            traces[t][c + 1, row] = (int(traces[t][c + 1, row]) + 1) % 3
        elif what == 1:                             # a flag: an active row dropped
            traces[t][c, row] = 0
        elif what == 2 and kind == 2:               # a multiplicity
            traces[t][c, row] += np.uint64(1)
        else:                                       # a filter set to 2
            traces[t][c, row] = 2
    return [member(bpg, random_table_program(kinds[t]), traces[t]) for t in range(n_tables)], links


@pytest.mark.parametrize("group", range(6))
def test_sixty_random_sets_agree_with_the_model_and_the_first_twenty_with_the_prover(bpg, group):
    verdicts = []
    for seed in range(10 * group, 10 * group + 10):
        members, links = random_set(bpg, 0x7000 + seed)
        got, want = checked(bpg, members, links)
        assert all(t.ok for t in got.tables), seed
        verdicts.append(got.ok)
        if seed < 20:
            assert prover_accepts(bpg, members, links) == got.ok, (seed, got.message)
    assert group != 0 or (True in verdicts and False in verdicts)


# ---------------------------------------------------------------------------------------------- 8. determinism


def test_the_report_is_a_function_of_the_set(bpg):
    """three calls (fresh challenges each), then the tables listed in another order with the links renamed"""
    members, links = two_looking_range_tables(bpg)
    members[2]["trace"][4, 9] += np.uint64(1)
    members[1]["trace"][0, 17] = 300                 # and a limb out of range on a row that may or may not send
    want = model.report(members, links)
    for _ in range(3):
        checked(bpg, members, links, want=want)
    order = [2, 0, 1]                                # new index -> old index
    new = {old: k for k, old in enumerate(order)}
    renamed = [([(new[t], p) for t, p in looking], (new[looked[0]], looked[1])) for looking, looked in links]
    got, _ = checked(bpg, [members[k] for k in order], renamed, want=want)
    assert not got.ok and "table %d" % new[2] in got.message
