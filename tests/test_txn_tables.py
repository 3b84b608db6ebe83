"""The host decisions about a transaction's seven tables (csrc/txn_tables.cpp) through bp_debug_txn_plan, without a GPU:
every case of txn_table_cases.py gives its status and message, and an accepted case the plan computed here from the
case -- the AIR, width, height and witness capacity of every table, the lookups that exist, the sponge rows whose XORs
the logic table holds first and the rows a seeded sponge table may absorb in."""
import ctypes as C

import pytest

import txn_table_cases as tc
from proof_protocol_decoder_amd._abi import TxnPlan as Plan

U32_MAX = 0xFFFFFFFF


@pytest.fixture(scope="module")
def env():
    from proof_protocol_decoder_amd import proof_gen as pg
    L = pg._bind()
    b = pg.ProverStateBuilder()
    for t, name in enumerate(pg.TABLES):
        getattr(b, "set_%s_circuit_size" % name)(range(tc.CFG["table_log_lo"][t], tc.CFG["table_log_hi"][t]))
    b.set(**{k: v for k, v in tc.CFG.items() if not k.startswith("table_")})
    return pg, L, b.cfg


def plan_of(env, case, words=None):
    """(status, message, plan) of bp_debug_txn_plan"""
    pg, L, cfg = env
    words = words or tc.ir_words(case)
    w, keep = tc.witness_struct(pg, case)
    plan = Plan()
    rc = L.bp_debug_txn_plan(C.byref(cfg), (C.c_uint64 * 25)(*words), 200, C.byref(w) if w is not None else None,
                             C.byref(plan))
    del keep
    return rc, L.bp_last_error().decode() if rc else "", plan


def check_plan(case, words, plan):
    from proof_protocol_decoder_amd import ops
    air = [tc.air_of(case.flags, t) for t in range(7)]
    for t in range(7):
        p, n = plan.table[t], 1 << case.log_n[t]
        assert (p.air_id, p.log_n, p.n_cols) == (air[t], case.log_n[t], words[18 + t]), (case.name, t)
        if air[t]:
            assert p.n_cols == ops.air_describe(air[t]).n_cols, (case.name, t)
        assert p.given == int(bool(air[t]) and t in (case.witness or {})), (case.name, t)
        assert p.capacity == ((n + 23) // 24 if t == 3 else n), (case.name, t)
        assert p.item_words == (0 if t == 2 else tc.item_words(t)), (case.name, t)
    active = []
    for i, (_, looking, looked) in enumerate(tc.PAIRS):
        lk = plan.lookup[i]
        assert ((lk.looking_table, lk.looking_air), (lk.looked_table, lk.looked_air)) == (looking, looked), i
        active.append(air[looking[0]] == looking[1] and air[looked[0]] == looked[1])
        assert lk.active == int(active[i]), (case.name, i)
    kf, _, sl = active
    covered = min(1 << case.log_n[4], (1 << case.log_n[5]) // 5) if sl else 0
    assert plan.logic_covered == covered, case.name
    assert plan.sponge_row_limit == min((1 << case.log_n[3]) // 24 if kf else U32_MAX, covered if sl else U32_MAX), case.name


@pytest.mark.parametrize("case", tc.ACCEPTED, ids=lambda c: c.name)
def test_an_accepted_case_gives_the_plan_computed_from_it(env, case):
    rc, msg, plan = plan_of(env, case)
    assert rc == tc.OK, msg
    check_plan(case, tc.ir_words(case), plan)


@pytest.mark.parametrize("case", tc.REFUSED, ids=lambda c: c.name)
def test_a_refused_case_gives_its_status_and_message(env, case):
    rc, msg, _ = plan_of(env, case)
    assert rc == case.status and case.match in msg, (rc, msg)


def test_the_decoded_entry_with_its_own_witness(env):
    case, words = tc.decoded_case()
    rc, msg, plan = plan_of(env, case, words)
    assert rc == tc.OK, msg
    check_plan(case, words, plan)
    assert [plan.table[t].given for t in (1, 3, 4, 6)] == [1, 1, 1, 1] and plan.lookup[0].active and plan.lookup[1].active


def test_the_sides_of_every_lookup_are_airs_of_their_tables(env):
    """air::ctl::pairs() names tables and AIRs in literals of its own: the flag that the header lists for a side's AIR
    must select that AIR at that side's table (the table's descriptor row lists it), and the pair then exists."""
    flag_of = {(t, air): f for f, (t, air, _) in tc.FLAGS.items()}
    for i, (name, looking, looked) in enumerate(tc.PAIRS):
        case = tc.Case(name, flag_of[looking] | flag_of[looked], tc.LOG_N, None, tc.OK, None)
        rc, msg, plan = plan_of(env, case)
        assert rc == tc.OK, msg
        lk = plan.lookup[i]
        assert plan.table[lk.looking_table].air_id == lk.looking_air and plan.table[lk.looked_table].air_id == lk.looked_air
        assert [plan.lookup[k].active for k in range(3)] == [int(k == i) for k in range(3)], name
        for f in (flag_of[looking], flag_of[looked]):   # one side synthetic: nothing to look up
            rc, msg, plan = plan_of(env, case._replace(flags=f))
            assert rc == tc.OK and not any(plan.lookup[k].active for k in range(3)), (name, msg)


def test_the_python_table_agrees_with_the_header_list():
    from proof_protocol_decoder_amd import proof_gen as pg
    rows = {(t, air, words) for _, t, air, _, _, words in pg.TXN_TABLE_AIRS}
    assert rows == set(tc.FLAGS.values()) and len(pg.TXN_TABLE_AIRS) == len(tc.FLAGS)
    for field, t, air, setter, members, words in pg.TXN_TABLE_AIRS:
        assert setter == "bp_ir_set_%s" % field and pg.WITNESS_FIELDS[t] == (*members, words)
