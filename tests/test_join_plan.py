"""``edm.join_plan``: the hand-over of a ragged batch inside one launch (dl_sample_chain_fc_join), on the CPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _c2():
    from difflinker_amd import synthetic
    data, _ = synthetic.make_batch('C2', seed=1000)
    return data['atom_mask'].squeeze(-1).sum(1).long().tolist(), data['linker_mask'].squeeze(-1).sum(1).long().tolist()


def test_join_plan_is_deterministic_and_pairs_split_plans_teams_with_finished_molecules():
    """Owners are exactly split_plan's teams; each helper is a molecule split_plan leaves on one compute unit, used once, and
    by the cost model done with its own chain before its owner's switch call; switch calls lie strictly inside the chain;
    every other molecule runs its whole chain alone."""
    from difflinker_amd.edm import forward_cost, join_plan, split_plan
    sizes, linkers = _c2()
    plan = join_plan(sizes, linkers, 501, 256, 6, 2)
    assert plan == join_plan(list(sizes), list(linkers), 501, 256, 6, 2)
    q_end, owners, helpers = plan
    assert sorted(owners) == sorted(split_plan(sizes, linkers, 501, 256, 6, 2)[1]) and len(owners) == 115
    assert len(helpers) == len(owners) == len(set(helpers)) and not set(helpers) & set(owners)
    c1 = [forward_cost(n, l, 6, 2, 1) for n, l in zip(sizes, linkers)]
    for o, hp in zip(owners, helpers):
        assert 0 < q_end[o] < 501
        assert 501 * c1[hp] <= q_end[o] * c1[o], (o, hp)
    assert all(q_end[b] == 501 for b in range(256) if b not in owners)
    # the owners with the most work get the helpers that finish first
    assert [c1[o] for o in owners] == sorted((c1[o] for o in owners), reverse=True)
    assert [c1[h] for h in helpers] == sorted(c1[h] for h in helpers)


def test_join_plan_predicts_the_c2_makespan_below_nine_tenths_of_one_launch():
    from difflinker_amd.edm import forward_cost, join_makespan, join_plan, split_plan
    sizes, linkers = _c2()
    single = max(forward_cost(n, l, 6, 2, 1) for n, l in zip(sizes, linkers)) * 501
    plan = join_plan(sizes, linkers, 501, 256, 6, 2)
    got = join_makespan(plan, sizes, linkers, 501, 6, 2) / single
    q_end, teams = split_plan(sizes, linkers, 501, 256, 6, 2)
    c1 = [forward_cost(n, l, 6, 2, 1) for n, l in zip(sizes, linkers)]
    two = (max(q * c for q, c in zip(q_end, c1)) + max((501 - q_end[b]) * forward_cost(sizes[b], linkers[b], 6, 2, 2)
                                                       for b in teams)) / single
    print(f'model makespan: join {got:.3f}, two launches {two:.3f} of one launch')
    assert got <= 0.90 and got < two


def test_join_plan_needs_split_plan_and_enough_finished_molecules():
    from difflinker_amd.edm import join_plan
    sizes, linkers = _c2()
    assert join_plan([50] * 256, [8] * 256, 501, 256, 6, 2) is None          # no split_plan
    assert join_plan(sizes + [40], linkers + [5], 501, 256, 6, 2) is None    # more molecules than compute units
    # two big molecules, one small one: split_plan puts both big ones on teams, one finished molecule is too few
    assert join_plan([50, 50, 20], [8, 8, 4], 25, 256, 2, 2) is None


def test_plans_of_the_batches_the_gpu_tests_name_their_routes_by():
    """tests/test_gpu_round5.py / test_gpu_join.py assert the route of every chain (``EDM.last_route``); the plans behind those
    routes, for one and two blocks on 256 and 304 compute units: the 12 molecules have a join_plan (six owners, six helpers ->
    'join'; three GCLs per block move the switch calls), the two batches of six have a split_plan and NO join_plan (four / five
    teams, two / one finished molecules -> 'two_launch')."""
    from difflinker_amd.edm import join_plan, split_plan
    T = 24
    twelve = ([50, 48, 50, 47, 20, 22, 18, 25, 21, 19, 23, 20], [8, 7, 9, 6, 4, 5, 3, 6, 4, 4, 5, 4])
    four_teams = ([50, 48, 50, 47, 20, 22], [8, 7, 9, 6, 4, 5])
    five_teams = ([55, 54, 53, 52, 30, 12], [9, 8, 8, 7, 5, 3])
    for L in (1, 2):
        for cus in (256, 304):
            q_end, owners, helpers = join_plan(*twelve, T + 1, cus, L, 2)
            assert (owners, helpers) == ([0, 1, 2, 3, 7, 10], [4, 5, 6, 8, 9, 11])
            assert q_end == [10, 10, 10, 10, 25, 25, 25, 22, 25, 25, 22, 25]
            assert sorted(split_plan(*twelve, T + 1, cus, L, 2)[1]) == owners
            q3, owners3, helpers3 = join_plan(*twelve, T + 1, cus, L, 3)
            assert (owners3, helpers3) == (owners, helpers) and q3 == [9, 9, 9, 9, 25, 25, 25, 21, 25, 25, 21, 25]
            assert split_plan(*four_teams, T + 1, cus, L, 2) == ([9, 9, 9, 9, 25, 25], [0, 1, 2, 3])
            assert join_plan(*four_teams, T + 1, cus, L, 2) is None
            assert split_plan(*five_teams, T + 1, cus, L, 2) == ([6, 6, 6, 6, 15, 25], [0, 1, 2, 3, 4])
            assert join_plan(*five_teams, T + 1, cus, L, 2) is None
