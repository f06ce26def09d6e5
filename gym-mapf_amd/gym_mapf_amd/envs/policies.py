"""Host helpers that build per-agent lookup-table policies for ``VecMapfEnv.set_policy('table', ...)``.

A table policy is what the reference's planning workflow ends with: every agent (or small group) is solved on its own
local view (``utils.get_local_view``) and the single-agent policies are joined.  A single-agent policy of a local view
is a function ``cell -> action``, i.e. one row of ``V`` bytes; the fused rollout follows ``table[rows[e, i], cell]``
for agent ``i`` of env ``e`` (include/mapf_hip.h, MAPF_POLICY_TABLE).

When a decomposing planner has found two agents in each other's way (``conflicting_pairs``) it merges them and replans the pair
on ``get_local_view(env, [i, j])``: that plan is a function of BOTH cells.  ``set_policy('joint', ...)`` follows it (include/mapf_hip.h,
MAPF_POLICY_JOINT): each merged agent has a ``[V, V]`` byte array indexed by (own cell, partner's cell).  ``pair_rows_from_policy``
and ``pair_shortest_path_rows`` build a pair's two arrays, ``join_plan`` lays solo rows and pair arrays out as the three arrays
``set_policy('joint')`` takes.  Nothing here needs a GPU.
"""
import itertools

import numpy as np

from gym_mapf_amd.envs import ACTIONS

_STAY = ACTIONS.index('STAY')
_MOVES = tuple(ACTIONS.index(name) for name in ('UP', 'RIGHT', 'DOWN', 'LEFT'))   # the tie-break order


def _distances(nbr, goal):
    """Breadth-first distance of every cell to ``goal`` over the noise-free moves (-1: the goal cannot be reached)."""
    V = nbr.shape[0]
    dist = np.full(V, -1, dtype=np.int64)
    dist[goal] = 0
    frontier = np.asarray([goal], dtype=np.int64)
    moves = nbr[:, list(_MOVES)].astype(np.int64)
    d = 0
    # moves are symmetric on a grid (a -> b by UP means b -> a by DOWN), so the cells that reach the frontier in one
    # move are the frontier's own neighbours
    while frontier.size:
        d += 1
        nxt = np.unique(moves[frontier].ravel())
        nxt = nxt[dist[nxt] < 0]
        dist[nxt] = d
        frontier = nxt
    return dist


def shortest_path_table(grid, goal_cells):
    """``(table uint8 [R, V], row_of_goal dict)`` for the DISTINCT cells of ``goal_cells`` (local ids, any shape), rows
    in ascending order of the goal id.  ``table[row_of_goal[g], c]`` is the first action in ACTIONS order (UP, RIGHT,
    DOWN, LEFT) whose noise-free target is one step closer to ``g`` by breadth-first distance over
    ``grid.tables()``'s neighbour table; STAY on the goal itself and on cells that cannot reach it."""
    _, _, nbr = grid.tables()
    V = nbr.shape[0]
    goals = np.unique(np.asarray(goal_cells, dtype=np.int64).ravel())
    if goals.size == 0 or goals.min() < 0 or goals.max() >= V:
        raise ValueError('goal_cells must be local ids 0..%d' % (V - 1))
    table = np.full((goals.size, V), _STAY, dtype=np.uint8)
    for r, goal in enumerate(goals):
        dist = _distances(nbr, int(goal))
        undecided = dist > 0
        for a in _MOVES:
            target = dist[nbr[:, a].astype(np.int64)]
            take = undecided & (target >= 0) & (target == dist - 1)
            table[r, take] = a
            undecided &= ~take
    return table, {int(g): r for r, g in enumerate(goals)}


def shortest_path_policy(env):
    """``(table, rows)`` for ``env.set_policy('table', table=table, rows=rows)``: every agent of a ``VecMapfEnv`` follows
    the shortest path to its own goal, ignoring the others.  ``rows`` is [A] when the env's goals are shared by all
    envs, else [E, A]."""
    table, row_of = shortest_path_table(env.grid, env.goal_local)
    lookup = np.zeros(table.shape[1], dtype=np.uint16)
    for goal, r in row_of.items():
        lookup[goal] = r
    rows = lookup[np.asarray(env.goal_local, dtype=np.int64)]
    if env._goal_bcast:
        rows = rows.reshape(-1)
    return table, np.ascontiguousarray(rows, dtype=np.uint16)


def row_from_policy(local_env, policy):
    """The table row uint8 [V] of a reference-style ``policy(s) -> a`` of a ONE-agent ``MapfEnv`` (for instance a
    ``get_local_view(env, [i])`` the caller planned on): ``row[c] = policy(c)`` -- with one agent the state integer is
    the cell's local id and the action integer the action code."""
    if local_env.n_agents != 1:
        raise ValueError('row_from_policy needs a one-agent env (a single-agent local view), got %d agents' % local_env.n_agents)
    V = len(local_env.valid_locations)
    row = np.empty(V, dtype=np.uint8)
    for c in range(V):
        a = int(policy(c))
        if not 0 <= a < len(ACTIONS):
            raise ValueError('policy(%d) = %d is not an action code 0..%d' % (c, a, len(ACTIONS) - 1))
        row[c] = a
    return row


def pair_rows_from_policy(local_env, policy):
    """The two arrays uint8 [V, V] ``(rows_0, rows_1)`` of a reference-style ``policy(s) -> a`` of a TWO-agent ``MapfEnv`` (for instance a
    ``get_local_view(env, [i, j])`` the caller planned on): ``rows_k[own cell, partner's cell]`` is agent k's action code.  States and
    actions are decoded through the env's own ``state_to_locations`` / ``integer_action_to_vector`` (agent 0 least significant)."""
    from gym_mapf_amd.envs.mapf_env import integer_action_to_vector
    if local_env.n_agents != 2:
        raise ValueError('pair_rows_from_policy needs a two-agent env (the local view of a merged pair), got %d agents' % local_env.n_agents)
    V = len(local_env.valid_locations)
    rows_0, rows_1 = np.empty((V, V), dtype=np.uint8), np.empty((V, V), dtype=np.uint8)
    for s in range(V * V):
        a = int(policy(s))
        if not 0 <= a < len(ACTIONS) ** 2:
            raise ValueError('policy(%d) = %d is not a joint action code 0..%d' % (s, a, len(ACTIONS) ** 2 - 1))
        c0, c1 = (local_env.loc_to_int[tuple(loc)] for loc in local_env.state_to_locations(s))
        a0, a1 = (ACTIONS.index(name) for name in integer_action_to_vector(a, 2))
        rows_0[c0, c1] = a0
        rows_1[c1, c0] = a1
    return rows_0, rows_1


def pair_shortest_path_rows(grid, goal_i, goal_j):
    """``(rows_i, rows_j)`` uint8 [V, V] for a pair merged on ``grid`` with goal cells ``goal_i``, ``goal_j`` (local ids): the noise-free
    shortest JOINT path.  Breadth-first search over the ``V * V`` joint cells (c_i, c_j) and the 25 joint actions; a move that makes a
    vertex conflict (both on one cell) or a swap is forbidden, and a joint cell with both agents on one cell is never entered.  In a
    joint cell the pair takes the first joint action in ``itertools.product(ACTIONS, repeat=2)`` order whose target is one step closer to
    the joint goal; STAY / STAY on the joint goal and on joint cells that cannot reach it.  ``rows_i[c_i, c_j]`` is agent i's action,
    ``rows_j[c_j, c_i]`` agent j's: each array is indexed by (own cell, partner's cell), as ``join_plan`` takes them."""
    _, _, nbr = grid.tables()
    nbr = np.asarray(nbr, dtype=np.int64)
    V = nbr.shape[0]
    goal_i, goal_j = int(goal_i), int(goal_j)
    if not (0 <= goal_i < V and 0 <= goal_j < V) or goal_i == goal_j:
        raise ValueError('goal_i and goal_j must be two different local ids 0..%d' % (V - 1))
    joint_actions = list(itertools.product(range(len(ACTIONS)), repeat=2))

    def targets(ci, cj, a_i, a_j):
        """the joint cell a joint action leads to, and whether the move is allowed"""
        ni, nj = nbr[ci, a_i], nbr[cj, a_j]
        return ni, nj, (ni != nj) & ~((ni == cj) & (nj == ci))

    # joint moves are symmetric (every allowed move has an allowed reverse), so the cells one move from the frontier are the
    # frontier's own targets
    dist = np.full(V * V, -1, dtype=np.int64)
    dist[goal_i * V + goal_j] = 0
    frontier = np.asarray([goal_i * V + goal_j], dtype=np.int64)
    d = 0
    while frontier.size:
        d += 1
        ci, cj = frontier // V, frontier % V
        found = []
        for a_i, a_j in joint_actions:
            ni, nj, ok = targets(ci, cj, a_i, a_j)
            found.append((ni * V + nj)[ok])
        nxt = np.unique(np.concatenate(found))
        nxt = nxt[dist[nxt] < 0]
        dist[nxt] = d
        frontier = nxt
    act_i = np.full(V * V, _STAY, dtype=np.uint8)
    act_j = np.full(V * V, _STAY, dtype=np.uint8)
    cells = np.arange(V * V, dtype=np.int64)
    ci, cj = cells // V, cells % V
    undecided = dist > 0
    for a_i, a_j in joint_actions:
        ni, nj, ok = targets(ci, cj, a_i, a_j)
        take = undecided & ok & (dist[ni * V + nj] == dist - 1)
        act_i[take] = a_i
        act_j[take] = a_j
        undecided &= ~take
    return act_i.reshape(V, V), np.ascontiguousarray(act_j.reshape(V, V).T)


def join_plan(V, n_agents, solo, pairs):
    """``(table uint8 [N], offsets uint32 [A], partners uint16 [A])`` for ``env.set_policy('joint', table=, offsets=, partners=)`` from a
    decomposed plan: ``solo`` is ``{agent: row uint8 [V]}`` (a row of ``shortest_path_table`` or ``row_from_policy``), ``pairs`` is
    ``{(i, j): (rows_i [V, V], rows_j [V, V])}`` (``pair_shortest_path_rows`` or ``pair_rows_from_policy``).  Every agent 0..A-1 appears
    exactly once.  The arrays are shared by all envs (the broadcast form)."""
    V, n_agents = int(V), int(n_agents)
    seen, segments = [], {}
    for agent, row in solo.items():
        row = np.asarray(row)
        if row.shape != (V,):
            raise ValueError('the row of solo agent %r must be [V] = (%d,), got %r' % (agent, V, row.shape))
        seen.append(int(agent))
        segments[int(agent)] = (row, int(agent))
    for (i, j), (rows_i, rows_j) in pairs.items():
        rows_i, rows_j = np.asarray(rows_i), np.asarray(rows_j)
        if rows_i.shape != (V, V) or rows_j.shape != (V, V):
            raise ValueError('the arrays of pair %r must both be [V, V] = (%d, %d), got %r and %r' % ((i, j), V, V, rows_i.shape, rows_j.shape))
        seen += [int(i), int(j)]
        segments[int(i)] = (rows_i, int(j))
        segments[int(j)] = (rows_j, int(i))
    for agent in seen:
        if not 0 <= agent < n_agents:
            raise ValueError('agent %d is not one of the %d agents' % (agent, n_agents))
        if seen.count(agent) > 1:
            raise ValueError('agent %d appears %d times in the plan' % (agent, seen.count(agent)))
    missing = sorted(set(range(n_agents)) - set(seen))
    if missing:
        raise ValueError('agent %d appears nowhere in the plan' % missing[0])
    offsets, partners, parts, at = np.zeros(n_agents, dtype=np.uint32), np.zeros(n_agents, dtype=np.uint16), [], 0
    for agent in range(n_agents):
        segment, partner = segments[agent]
        if segment.size and (segment.min() < 0 or segment.max() >= len(ACTIONS)):
            raise ValueError('the plan of agent %d holds a value that is not an action code 0..%d' % (agent, len(ACTIONS) - 1))
        offsets[agent], partners[agent] = at, partner
        parts.append(np.ascontiguousarray(segment, dtype=np.uint8).ravel())
        at += segment.size
        if at > 0x7FFFFFFF:
            raise ValueError('the joint table exceeds 2**31 - 1 bytes')
    return np.concatenate(parts), offsets, partners


GROUP_PAD = 0xFFFF        # the cell of a padded position of a group's key (include/mapf_hip.h MAPF_POLICY_GROUP)


def group_entries_from_policy(local_env, policy, states):
    """``(cells uint16 [n, 4], actions uint8 [n, 4])``: the book entries of a reference-style ``policy(s) -> a`` of a G-agent ``MapfEnv``,
    G = 2..4 (for instance a ``get_local_view(env, [i, j, k])`` the caller planned on), for the state integers ``states`` the planner
    visited -- one entry each, in their order.  States and actions are decoded as ``pair_rows_from_policy`` decodes them (agent 0 least
    significant); positions G..3 are padded (cell 0xFFFF, action 0).  The view's agents must be in ascending order of the env's."""
    from gym_mapf_amd.envs.mapf_env import integer_action_to_vector
    G = local_env.n_agents
    if not 2 <= G <= 4:
        raise ValueError('group_entries_from_policy needs an env of 2..4 agents (the local view of a merged group), got %d agents' % G)
    states = [int(s) for s in states]
    cells, actions = np.full((len(states), 4), GROUP_PAD, dtype=np.uint16), np.zeros((len(states), 4), dtype=np.uint8)
    for n, s in enumerate(states):
        a = int(policy(s))
        if not 0 <= a < len(ACTIONS) ** G:
            raise ValueError('policy(%d) = %d is not a joint action code 0..%d' % (s, a, len(ACTIONS) ** G - 1))
        cells[n, :G] = [local_env.loc_to_int[tuple(loc)] for loc in local_env.state_to_locations(s)]
        actions[n, :G] = [ACTIONS.index(name) for name in integer_action_to_vector(a, G)]
    return cells, actions


def group_shortest_path_entries(grid, goals, region):
    """``(cells uint16 [n, 4], actions uint8 [n, 4])``: the book of a group of G = 2..4 agents merged on ``grid`` with goal cells ``goals``
    (local ids, in the members' order), replanned on ``region`` (a list of distinct local ids): the noise-free
    shortest JOINT path, ``pair_shortest_path_rows``' breadth-first search for G goals, restricted to the joint cells whose members all
    stand in ``region``.  A move that makes a vertex conflict or a swap between any two members, or leaves the region, is forbidden.
    There is one entry per joint cell of distinct region cells; in it the group takes the first joint action in
    ``itertools.product(range(5), repeat=G)`` order whose target is one step closer to the joint goal, STAY for all members on the
    joint goal and where the joint goal cannot be reached inside the region (everywhere, when a goal lies outside it).  Positions G..3
    are padded (cell 0xFFFF, action 0).
    Refuses ``len(region) ** G > 2**22``."""
    _, _, nbr = grid.tables()
    nbr = np.asarray(nbr, dtype=np.int64)
    V = nbr.shape[0]
    goals, region = [int(g) for g in goals], np.asarray(region, dtype=np.int64).reshape(-1)
    G, R = len(goals), int(region.size)
    if not 2 <= G <= 4:
        raise ValueError('a group has 2..4 members, got %d goals' % G)
    if R == 0 or region.min() < 0 or region.max() >= V or np.unique(region).size != R:
        raise ValueError('region must be distinct local ids 0..%d' % (V - 1))
    if R ** G > 2 ** 22:
        raise ValueError('the region of %d cells has %d ** %d joint cells, above 2**22' % (R, R, G))
    if len(set(goals)) != G or not all(0 <= g < V for g in goals):
        raise ValueError('goals must be %d different local ids 0..%d' % (G, V - 1))
    where = np.full(V, -1, dtype=np.int64)
    where[region] = np.arange(R)
    step = where[nbr[region]]                          # [R, 5]: the region index an action leads to, -1 outside the region
    joint_actions = list(itertools.product(range(len(ACTIONS)), repeat=G))

    def digits(idx):
        """the members' region indices of joint cells, member 0 most significant"""
        out = []
        for k in range(G):
            out.append((idx // R ** (G - 1 - k)) % R)
        return out

    def targets(c, acts):
        """the joint cell a joint action leads to, and whether the move is allowed"""
        n = [step[c[k], acts[k]] for k in range(G)]
        ok = np.ones(c[0].shape, dtype=bool)
        for k in range(G):
            ok &= n[k] >= 0
        for a, b in itertools.combinations(range(G), 2):
            ok &= (n[a] != n[b]) & ~((n[a] == c[b]) & (n[b] == c[a]))
        idx = np.zeros(c[0].shape, dtype=np.int64)
        for k in range(G):
            idx = idx * R + np.maximum(n[k], 0)
        return idx, ok

    # joint moves are symmetric (every allowed move has an allowed reverse), so the cells one move from the frontier are its own targets
    dist = np.full(R ** G, -1, dtype=np.int64)
    frontier, d = np.zeros(0, dtype=np.int64), 0
    if all(where[g] >= 0 for g in goals):                # (a goal outside the region cannot be reached inside it)
        goal_idx = 0
        for g in goals:
            goal_idx = goal_idx * R + int(where[g])
        dist[goal_idx] = 0
        frontier = np.asarray([goal_idx], dtype=np.int64)
    while frontier.size:
        d += 1
        c = digits(frontier)
        found = []
        for acts in joint_actions:
            idx, ok = targets(c, acts)
            found.append(idx[ok])
        nxt = np.unique(np.concatenate(found))
        nxt = nxt[dist[nxt] < 0]
        dist[nxt] = d
        frontier = nxt
    every = np.arange(R ** G, dtype=np.int64)
    c = digits(every)
    distinct = np.ones(every.shape, dtype=bool)
    for a, b in itertools.combinations(range(G), 2):
        distinct &= c[a] != c[b]
    every, c = every[distinct], [x[distinct] for x in c]
    acted = np.zeros((every.size, G), dtype=np.uint8)
    undecided = dist[every] > 0
    for acts in joint_actions:
        idx, ok = targets(c, acts)
        take = undecided & ok & (dist[idx] == dist[every] - 1)
        acted[take] = acts
        undecided &= ~take
    cells, actions = np.full((every.size, 4), GROUP_PAD, dtype=np.uint16), np.zeros((every.size, 4), dtype=np.uint8)
    for k in range(G):
        cells[:, k] = region[c[k]]
    actions[:, :G] = acted
    return cells, actions


def join_group_plan(V, n_agents, solo, groups):
    """The arrays of ``env.set_policy('group', **plan)`` -- a dict ``table`` uint8 [A, V], ``rows`` uint16 [A], ``members`` uint16 [A, 4],
    ``book`` uint32 [A], ``entry_cells`` uint16 [N, 4], ``entry_actions`` uint8 [N, 4], ``book_begin`` uint32 [n_books + 1] -- from a
    decomposed plan: ``solo`` is ``{agent: row uint8 [V]}`` for EVERY agent 0..A-1 (a row of ``shortest_path_table`` or
    ``row_from_policy``: what the agent does where its group's book has no entry), ``groups`` is ``{(i, j, ...): (cells [n, 4],
    actions [n, 4])}`` with 2..4 ascending agents per key (``group_shortest_path_entries`` or ``group_entries_from_policy``, position p
    of an entry being the key's p-th agent).  An agent appears in at most one group.  The arrays are shared by all envs (the broadcast
    form); group k of ``groups`` gets book k."""
    V, n_agents = int(V), int(n_agents)
    if sorted(int(a) for a in solo) != list(range(n_agents)):
        raise ValueError('solo must hold one row for every agent 0..%d' % (n_agents - 1))
    table = np.zeros((n_agents, V), dtype=np.uint8)
    for agent, row in solo.items():
        row = np.asarray(row)
        if row.shape != (V,):
            raise ValueError('the row of agent %r must be [V] = (%d,), got %r' % (agent, V, row.shape))
        if row.size and (row.min() < 0 or row.max() >= len(ACTIONS)):
            raise ValueError('the row of agent %d holds a value that is not an action code 0..%d' % (agent, len(ACTIONS) - 1))
        table[int(agent)] = row
    members = np.full((n_agents, 4), GROUP_PAD, dtype=np.uint16)
    members[:, 0] = np.arange(n_agents)
    book, begin, all_cells, all_actions, seen = np.zeros(n_agents, dtype=np.uint32), [0], [], [], set()
    for k, (key, (cells, actions)) in enumerate(groups.items()):
        key = tuple(int(a) for a in key)
        cells, actions = np.asarray(cells), np.asarray(actions)
        if not 2 <= len(key) <= 4 or list(key) != sorted(set(key)):
            raise ValueError('a group is 2..4 different agents in ascending order, got %r' % (key,))
        if key[0] < 0 or key[-1] >= n_agents:
            raise ValueError('group %r names an agent that is not one of the %d agents' % (key, n_agents))
        if seen & set(key):
            raise ValueError('agent %d appears in two groups' % sorted(seen & set(key))[0])
        seen |= set(key)
        if cells.ndim != 2 or cells.shape[1] != 4 or actions.shape != cells.shape:
            raise ValueError('the entries of group %r must be two [n, 4] arrays, got %r and %r' % (key, cells.shape, actions.shape))
        G = len(key)
        if cells.size and ((cells[:, :G] >= V).any() or (cells[:, G:] != GROUP_PAD).any() or (actions > 4).any() or (actions[:, G:] != 0).any()):
            raise ValueError('the entries of group %r must hold %d cells below V = %d and action codes 0..4, padded with 0xFFFF and 0' % (key, G, V))
        for agent in key:
            members[agent, :G], members[agent, G:], book[agent] = key, GROUP_PAD, k
        all_cells.append(cells.astype(np.uint16))
        all_actions.append(actions.astype(np.uint8))
        begin.append(begin[-1] + cells.shape[0])
    if begin[-1] > 1 << 24:
        raise ValueError('the plan holds %d entries, above 2**24' % begin[-1])
    return dict(table=table, rows=np.arange(n_agents, dtype=np.uint16), members=members, book=book,
                entry_cells=np.concatenate(all_cells) if all_cells else np.zeros((0, 4), np.uint16),
                entry_actions=np.concatenate(all_actions) if all_actions else np.zeros((0, 4), np.uint8), book_begin=np.asarray(begin, dtype=np.uint32))


def evaluate(env, n_episodes, max_steps, chunk=256, log=False):
    """Monte-Carlo evaluation of whatever drives ``env``'s ``rollout(actions=None)`` -- a table policy, a joint table policy (a plan with
    merged pairs, ``join_plan``), a group policy (a plan with merged groups of up to four, ``join_group_plan``), the greedy policy or the random stream: EXACTLY ``n_episodes`` episodes of at most ``max_steps`` steps in every env of a ``VecMapfEnv``, inside
    totals-only fused rollouts.  Sets the episode limit and the episode budget (``set_episode_limit``, ``set_episode_budget``; both
    stay set), resets, then issues ``ceil(n_episodes * max_steps / chunk)`` launches of ``chunk`` steps that accumulate into one set
    of totals.  Every episode ends within ``max_steps`` steps, so after that many steps every env is parked by construction: nothing
    is polled, and ``episodes_left().max() == 0`` is asserted at the end.  Returns a dict of host arrays, one value per env:
    ``returns`` f64 (the rewards of the ``n_episodes`` episodes, no cut-off episode among them), ``goal_ends`` (= episodes -
    collisions: episodes that ended on the goals, a terminal start state included), ``collisions``, ``truncations`` and
    ``live_steps`` (the steps those episodes took), uint32 -- ``goal_ends + collisions + truncations == n_episodes`` everywhere.
    On an env that counts conflicting pairs (``set_conflict_pairs``) the matrix is zeroed before the first launch and returned as
    ``pair_conflicts`` uint64 [n_slots, A, A] (``conflicts`` and ``conflicting_pairs`` read it): which agents got in each other's
    way during those episodes.  With ``log=True`` the episodes themselves come back too (``set_episode_log(n_episodes)``, which stays
    set; the log is cleared before the first launch and ``count == n_episodes`` is asserted everywhere): ``episode_returns`` f64,
    ``episode_steps`` uint32 and ``episode_outcomes`` uint8 (1 on the goals, 3 by a collision, 4 truncated), each [E, n_episodes] in
    the order the episodes ended -- ``episode_statistics`` reads them.  Not covered: the multi-map and union-map wrappers and the scalar ``MapfEnv``."""
    n_episodes, max_steps, chunk = int(n_episodes), int(max_steps), int(chunk)
    if n_episodes < 1 or max_steps < 1 or chunk < 1:
        raise ValueError('evaluate needs n_episodes >= 1, max_steps >= 1 and chunk >= 1')
    env.set_episode_limit(max_steps)
    env.set_episode_budget(n_episodes)
    if log:
        env.set_episode_log(n_episodes)            # (every call empties the log and drops the partial sums)
    env.reset()
    counting = bool(getattr(env, 'conflict_slots', 0))
    if counting:
        cleared = env.conflict_pairs(zero=True)   # (kept until the sync below: in device mode the read is only enqueued)
    totals = None
    for _ in range(-(-n_episodes * max_steps // chunk)):
        totals = env.rollout(chunk, auto_reset=True, accumulate_into=totals)
    env.sync()
    host = lambda a: a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
    left = host(env.episodes_left())
    env.sync()
    assert int(left.max(initial=0)) == 0, 'after n_episodes * max_steps steps every env is parked'
    out = {k: host(totals[k]) for k in ('returns', 'collisions', 'truncations', 'live_steps')}
    out['goal_ends'] = host(totals['episodes']) - out['collisions']
    if counting:
        del cleared
        pairs = env.conflict_pairs()
        env.sync()
        out['pair_conflicts'] = host(pairs)
    if log:
        episodes = env.episode_log()
        env.sync()
        assert (host(episodes['count']) == n_episodes).all(), 'every env has ended exactly n_episodes episodes'
        out['episode_returns'], out['episode_steps'] = host(episodes['returns']), host(episodes['steps'])
        out['episode_outcomes'] = host(episodes['outcome'])
    return out


def episode_statistics(log):
    """Host-side statistics of an episode log: ``log`` is what ``evaluate(..., log=True)`` returns (``episode_returns``,
    ``episode_steps``, ``episode_outcomes``), or what ``VecMapfEnv.episode_log`` returns (``returns``, ``steps``, ``outcome`` and
    ``count``: then only the first ``min(count, C)`` columns of an env are read).  Returns ``{'per_env': {...}, 'pooled': {...}}``;
    per env the values are arrays [E], pooled over all logged episodes they are scalars: ``n`` (episodes read), ``mean``, ``std``
    (the SAMPLE standard deviation, ddof = 1; nan below two episodes) and ``stderr`` (= std / sqrt(n)) of the episode returns,
    ``goal_share``, ``collision_share`` and ``truncated_share`` (outcomes 1, 3 and 4 -- they sum to 1), ``mean_steps`` and
    ``max_steps`` (0 without an episode)."""
    host = lambda a: np.asarray(a.cpu() if hasattr(a, 'cpu') else a)
    pick = lambda *names: next(host(log[n]) for n in names if n in log)
    returns = pick('episode_returns', 'returns').astype(np.float64, copy=False)
    steps, outcome = pick('episode_steps', 'steps').astype(np.int64), pick('episode_outcomes', 'outcome').astype(np.int64)
    if returns.ndim != 2 or steps.shape != returns.shape or outcome.shape != returns.shape:
        raise ValueError('an episode log holds three [E, C] arrays, got shapes %r, %r, %r' % (returns.shape, steps.shape, outcome.shape))
    E, C = returns.shape
    n = np.minimum(host(log['count']).astype(np.int64), C) if 'count' in log else np.full(E, C, np.int64)
    if n.shape != (E,):
        raise ValueError('count must be [E]')
    valid = np.arange(C)[None, :] < n[:, None]

    def stats(valid, axis):
        k = valid.sum(axis=axis)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = np.where(valid, returns, 0.0).sum(axis=axis) / k
            centred = np.where(valid, returns - (mean[:, None] if axis == 1 else mean), 0.0)
            std = np.sqrt((centred * centred).sum(axis=axis) / (k - 1))
            std = np.where(k > 1, std, np.nan)
            share = lambda code: (valid & (outcome == code)).sum(axis=axis) / k
            res = {'n': k, 'mean': mean, 'std': std, 'stderr': std / np.sqrt(k), 'goal_share': share(1), 'collision_share': share(3),
                   'truncated_share': share(4), 'mean_steps': np.where(valid, steps, 0).sum(axis=axis) / k,
                   'max_steps': np.where(valid, steps, 0).max(axis=axis, initial=0)}
        return res if axis == 1 else {key: (int(v) if key in ('n', 'max_steps') else float(v)) for key, v in res.items()}

    return {'per_env': stats(valid, 1), 'pooled': stats(valid, None)}


def conflicts(M):
    """The count per UNORDERED agent pair of a conflict matrix ``M`` [..., A, A] (``VecMapfEnv.conflict_pairs``): vertex conflicts
    (the upper triangle) plus swaps (the lower one), as a symmetric matrix of the same shape with a zero diagonal."""
    M = np.asarray(M.cpu() if hasattr(M, 'cpu') else M, dtype=np.uint64)
    if M.ndim < 2 or M.shape[-1] != M.shape[-2]:
        raise ValueError('a conflict matrix is [..., A, A], got shape %r' % (M.shape,))
    upper, lower = np.triu(M, 1), np.tril(M, -1)
    both = upper + np.swapaxes(lower, -1, -2)
    return both + np.swapaxes(both, -1, -2)


def conflicting_pairs(M):
    """The rows ``(i, j, vertex, swap)``, i < j, of the agent pairs with a nonzero count in the conflict matrix ``M`` [A, A] or
    [n_slots, A, A] (the slots are summed), sorted by (i, j): the pairs a decomposing planner merges into one group and replans."""
    M = np.asarray(M.cpu() if hasattr(M, 'cpu') else M, dtype=np.uint64)
    if M.ndim == 3:
        M = M.sum(axis=0, dtype=np.uint64)
    if M.ndim != 2 or M.shape[0] != M.shape[1]:
        raise ValueError('a conflict matrix is [A, A] or [n_slots, A, A], got shape %r' % (M.shape,))
    vertex, swap = np.triu(M, 1), np.tril(M, -1).T
    return [(int(i), int(j), int(vertex[i, j]), int(swap[i, j])) for i, j in zip(*np.nonzero(vertex + swap))]


def conflicting_groups(M, max_size=4):
    """``(groups, too_large)``: the connected components of the conflict graph of the matrix ``M`` [A, A] or [n_slots, A, A] (the slots
    are summed) -- two agents are joined when they have a nonzero count, vertex or swap -- as sorted tuples of agents, each list sorted.
    ``groups`` holds the components of 2..``max_size`` agents: what a decomposing planner merges, replans on a region
    (``group_shortest_path_entries``) and hands to ``join_group_plan``; components above ``max_size`` come back in ``too_large``.  Agents
    without a conflict are in neither list."""
    A = np.asarray(M).shape[-1]
    parent = list(range(A))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i, j, _, _ in conflicting_pairs(M):
        parent[find(j)] = find(i)
    components = {}
    for a in range(A):
        components.setdefault(find(a), []).append(a)
    found = sorted(tuple(c) for c in components.values() if len(c) >= 2)
    return [c for c in found if len(c) <= max_size], [c for c in found if len(c) > max_size]
