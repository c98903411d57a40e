"""CPU: tickets with different search sets on ONE resident database, through the drop-in's own methods (ticket.py, hyperparameter.py)
over the numpy stand-in with search sets (tests/_standin_views.py) on the reference's golden vectors.  Under test is everything the
Python layers add: the immutable view a round binds to, positions in place of rows in every map and row list, the hand-back of the
handle between tickets with different sets.  The GPU twin is tests/test_search_set_gpu.py."""
import numpy as np
import pytest

from _helpers import DEFAULT_WEIGHTS, SEED, STREAMS, golden_json, golden_npy, records_from_dense


def _golden(name):
    g = golden_json(name + ".json")
    x = golden_npy(name + "_x.npy")
    ids = np.asarray(g.get("clip_ids") or g["clip_order"], dtype=np.int64)
    return g, x, ids


def test_two_tickets_with_their_own_search_sets_share_one_database():
    import video_query_algorithms_amd as vqa
    from _search_set_cases import check_two_tickets
    from _standin_views import ViewOracleFeatureDB
    g, x, ids = _golden("real_subset")
    recs = records_from_dense(x, ids, [1, 2, 3])
    shared = ViewOracleFeatureDB(x, clip_ids=ids)
    check_two_tickets(vqa, shared, lambda rows: ViewOracleFeatureDB(x[rows], clip_ids=ids[rows]), recs, x, ids, g, STREAMS,
                      DEFAULT_WEIGHTS, SEED)
    assert shared._in_use is None and not shared._sets


def test_a_ticket_without_a_defined_set_scans_the_whole_database_and_switches_nothing():
    import video_query_algorithms_amd as vqa
    from _search_set_cases import same_round, ticket_round
    from _standin_views import ViewOracleFeatureDB
    g, x, ids = _golden("real_subset")
    recs = records_from_dense(x, ids, [1, 2, 3])
    lab = g["labelled"]
    plain = ticket_round(vqa, ViewOracleFeatureDB(x, clip_ids=ids), recs, g["ref_clip_id"], 1, g["user_matches"], lab, STREAMS, DEFAULT_WEIGHTS, SEED)
    db = ViewOracleFeatureDB(x, clip_ids=ids)
    db.define_search_set("other", ids[:5])
    got = ticket_round(vqa, db, recs, g["ref_clip_id"], 1, g["user_matches"], lab, STREAMS, DEFAULT_WEIGHTS, SEED)    # set 1 is not defined
    assert same_round(got, plain) and list(got["scores"].keys()) == ids.tolist() and db.use_calls == 0
    got = ticket_round(vqa, db, recs, g["ref_clip_id"], ["unhashable"], g["user_matches"], lab, STREAMS, DEFAULT_WEIGHTS, SEED)
    assert same_round(got, plain) and db.use_calls == 0


def test_view_object():
    from video_query_algorithms_amd.feature_db import SearchSetView
    from _standin_views import ViewOracleFeatureDB
    x = np.zeros((6, 1, 1, 4), dtype=np.float32)
    db = ViewOracleFeatureDB(x, clip_ids=[50, 40, 30, 20, 10, 60])
    v = db.define_search_set("s", [10, 50, 30, 10, 50])               # any order, duplicates collapse -> ascending rows
    assert isinstance(v, SearchSetView) and v.rows.tolist() == [0, 2, 4] and v.clip_ids.tolist() == [50, 30, 10] and v.n == 3
    assert [v.row_of(c) for c in (50, 30, 10)] == [0, 1, 2] and v.has_clip("30") and not v.has_clip(40) and not v.has_clip("x")
    with pytest.raises(KeyError):
        v.row_of(40)
    with pytest.raises(AttributeError):
        v.n = 4
    with pytest.raises(ValueError):
        v.rows[0] = 1
    with pytest.raises(KeyError):
        db.define_search_set("t", [10, 11])                           # an id the database does not hold
    assert not db.has_search_set("t")
    w = db.use_search_set(None)
    assert w.set_id is None and w.n == 6 and w.row_of(20) == 3 and w.clip_ids is db.clip_ids and w.rows.tolist() == list(range(6))
    assert db.use_search_set("s") is v and db.use_search_set("s") is v and db.use_calls == 1
