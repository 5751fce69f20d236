"""The split-producer rollout kernel's tick chain, script by script.  Its transition wave keeps
two parity buffers of every env's grid and inventory rows and brings the older one up to date
from a record of the last tick's change (one cleared cell, or a restart with its list of cleared
cells); on 3x3 32-env tiles at 512 threads its scatter runs on two waves, four lanes per env.
Each script below is built so that a value carried from one tick to the next (the facing cell
and the move target's kind, the inventory row, the cleared cells and their kinds), gone stale in
either buffer, changes a result; they hold for any implementation that carries such values,
whether it re-reads them from LDS or keeps them in registers.

Every case is a hand-made 12x12 single-scenario pool with given actions, 30 ticks, and is compared
bit for bit with the CPU variant (itself pinned to the oracle) and with 30 craft_step calls:
observation / reward / done / success rings, get_state(), stats(), and a clean check().  Sizes:
n = 1 (a lone env), 33 (one env past a 32-env tile) and 70 (full tiles and a partial one); the 30
ticks in one launch and again as 5 + 1 + 9 + 15; rings of 3 and 32 slots; the default shape, the
continuous pipeline (chunk -1) and 16-env tiles on 320 threads."""
import numpy as np
import pytest
import torch

from psketch_amd import CraftSim
from psketch_amd import _native as N
from tests.test_gpu_recipes import chained_recipes, triple_recipes

pytestmark = pytest.mark.gpu

WORLD, W, T, NMAX = "craft_medium_12x12", 12, 30, 72
SHAPES = {"default": None, "continuous": (32, 512, -1), "tile16": (16, 320, 0)}
LAUNCHES = ((30,), (5, 1, 9, 15))
RINGS = (3, 32)
D, U, L, R, USE, STOP = N.DOWN, N.UP, N.LEFT, N.RIGHT, N.USE, N.STOP


def _sim(case, n, device):
    sim = CraftSim(WORLD, n_envs=n, device=device, pool_capacity=1, recipes=case["recipes"])
    sim.load_pool(case["grid"][None])
    return sim


def _start(sim, case, n):
    """Slots 0..n-1 := the case's first n envs: spec (the restart pose), agent, inventory."""
    x, y, d, task = (case[k][:n] for k in ("x", "y", "dir", "task"))
    spec = np.stack([np.zeros(n, dtype=np.int32), x, y, d, task], 1).astype(np.int32)
    agent = np.stack([x, y, d, np.full(n, 40)], 1).astype(np.int32)
    sim.set_state(spec, agent, case["inv"][:n, :sim.n_kinds].astype(np.int32))


def _base(recipes=None):
    sim = CraftSim(WORLD, n_envs=1, device="cpu", pool_capacity=1, recipes=recipes)
    ix, tm = sim.cookbook.index, sim.task_manager
    grid = np.zeros((W, W), dtype=np.uint8)
    grid[0, :] = grid[-1, :] = grid[:, 0] = grid[:, -1] = ix["boundary"]
    return ix, tm, grid, sim.n_kinds


def _case(recipes, grid, rows, autoreset=True):
    """rows: one dict per env type (x, y, dir, task, inv {kind id: count}, script); env i is of
    type i % len(rows) and repeats its script."""
    n = NMAX
    c = dict(recipes=recipes, grid=grid, autoreset=autoreset, inv=np.zeros((n, N.MAX_KINDS), dtype=np.int32),
             acts=np.empty((T, n), dtype=np.int32))
    for k in ("x", "y", "dir", "task"):
        c[k] = np.empty(n, dtype=np.int32)
    for i in range(n):
        r = rows[i % len(rows)](i // len(rows)) if callable(rows[i % len(rows)]) else rows[i % len(rows)]
        assert grid[r["x"], r["y"]] == 0
        c["x"][i], c["y"][i], c["dir"][i], c["task"][i] = r["x"], r["y"], r["dir"], r["task"]
        for k, v in r.get("inv", {}).items():
            c["inv"][i, k] = v
        c["acts"][:, i] = [r["script"][t % len(r["script"])] for t in range(T)]
    return c


def _neighbours():
    """Carried neighbour kinds (and the remembered kinds of cleared cells).  Each env starts at
    (1, y) facing +x and restarts there on STOP:
    0 grabs the wood at (2, 1) and walks into the cell it just cleared (stale neighbours: the move
      is blocked); after the restart the wood is back and blocks two moves (stale: the agent walks
      through it; kinds restored from a stale record: the cell stays empty or holds another kind);
    1 bridges the water at (2, 3) with its one bridge and crosses; after the restart the inventory
      is empty, the water is back, USE does nothing and the moves are blocked;
    2 the same with an axe and the stone at (2, 5);
    3 turns towards the boundary without moving, USEs (nothing), turns towards the wood at (1, 8)
      without moving, STOPs facing it (go[wood] is satisfied only with the neighbour of the new
      direction), then grabs it, walks into the cell and back;
    4 clears five wood cells of (2..7, 9) before its STOP, more than the cleared-cell list holds,
      so the restart restores the whole row; then the first move is blocked by the restored wood."""
    ix, tm, grid, _ = _base()
    grid[2, 1] = ix["wood"]
    grid[2, 3] = ix["water"]
    grid[2, 5] = ix["stone"]
    grid[1, 8] = ix["wood"]
    grid[2:8, 9] = ix["wood"]
    get, go = tm["get[wood]"].id, tm["go[wood]"].id
    cross = [USE, R, R, STOP, R, USE, R, STOP]
    rows = [lambda j: dict(x=1, y=1, dir=N.RIGHT, task=go if j % 2 else get, script=[USE, R, R, STOP, R, R, USE, STOP]),
            dict(x=1, y=3, dir=N.RIGHT, task=tm["make[bridge]"].id, inv={ix["bridge"]: 1}, script=cross),
            dict(x=1, y=5, dir=N.RIGHT, task=tm["make[axe]"].id, inv={ix["axe"]: 1}, script=cross),
            lambda j: dict(x=1, y=7, dir=N.RIGHT, task=go if j % 2 == 0 else get,
                           script=[L, USE, U, STOP, U, USE, U, D, STOP]),
            dict(x=1, y=9, dir=N.RIGHT, task=get, script=[USE, R] * 5 + [STOP, R, USE, R, USE, R, STOP])]
    return _case(None, grid, rows)


def _inventory(autoreset):
    """The inventory row from tick to tick.
    0 grabs wood, iron, grass, wood, gold along (2..6, 1): several kinds, a count of two, all zero
      again after the restart (a stale row: counts carried into the next episode);
    1 get[wood]: USE, STOP, STOP: the first STOP comes on the tick after the count changed and must
      succeed, the second right after the restart and must not;
    2 make[plank] at a workshop with two woods: USE, STOP (made), then, the inventory emptied by
      the restart, USE (nothing to craft from), STOP (not made), STOP;
    3 get[iron]: grabs, walks on and back, STOPs;
    4 holds many kinds and only walks: the row is carried unchanged until its STOP.
    Without auto-reset the first STOP freezes the env: done stays 1, success keeps being evaluated
    on the frozen state's inventory, and the state no longer changes."""
    ix, tm, grid, K = _base()
    for x, k in zip(range(2, 7), ("wood", "iron", "grass", "wood", "gold")):
        grid[x, 1] = ix[k]
    grid[2, 3] = ix["wood"]
    grid[2, 5] = ix["workshop0"]
    grid[2, 7] = ix["iron"]
    rows = [dict(x=1, y=1, dir=N.RIGHT, task=tm["get[grass]"].id, script=[USE, R] * 5 + [STOP]),
            dict(x=1, y=3, dir=N.RIGHT, task=tm["get[wood]"].id, script=[USE, STOP, STOP]),
            dict(x=1, y=5, dir=N.RIGHT, task=tm["make[plank]"].id, inv={ix["wood"]: 2},
                 script=[USE, STOP, USE, STOP, STOP]),
            dict(x=1, y=7, dir=N.RIGHT, task=tm["get[iron]"].id, script=[USE, R, L, STOP]),
            dict(x=1, y=9, dir=N.RIGHT, task=tm["make[bed]"].id, inv={k: 1 + k % 5 for k in range(7, K)},
                 script=[U, U, D, R, L, D, STOP])]
    return _case(None, grid, rows, autoreset)


def _recipes(recipes):
    """A workshop's USE, with chained_recipes() and with triple_recipes() (a three-ingredient recipe).
    0 workshop0 with wood, iron, grass: plank, then (chained) axe from the plank just made in the
      same USE, then rope; the later USEs run the counts down until an ingredient lacks;
    1 workshop0 with wood only: plank, but the axe lacks its iron;
    2 workshop1 with wood, stick, iron, plank, grass: stick from itself (yield 3 when chained), bed
      (two or three ingredients), shears;
    3 workshop0 with nothing: every USE lacks every ingredient;
    4 workshop2 with wood, iron, plank, stick, grass: cloth, bridge, ladder."""
    ix, tm, grid, _ = _base(recipes)
    for y, k in ((1, "workshop0"), (3, "workshop0"), (5, "workshop1"), (7, "workshop0"), (9, "workshop2")):
        grid[2, y] = ix[k]
    s = [L, R, USE, USE, USE, R, STOP]                    # (the turns are blocked: boundary, workshop)
    rows = [dict(x=1, y=1, dir=N.RIGHT, task=tm["make[axe]"].id, inv={ix["wood"]: 2, ix["iron"]: 1, ix["grass"]: 3}, script=s),
            dict(x=1, y=3, dir=N.RIGHT, task=tm["make[plank]"].id, inv={ix["wood"]: 1}, script=s),
            dict(x=1, y=5, dir=N.RIGHT, task=tm["make[shears]"].id,
                 inv={ix["wood"]: 2, ix["stick"]: 1, ix["iron"]: 2, ix["plank"]: 1, ix["grass"]: 1}, script=s),
            dict(x=1, y=7, dir=N.RIGHT, task=tm["make[rope]"].id, script=s),
            dict(x=1, y=9, dir=N.RIGHT, task=tm["make[bridge]"].id,
                 inv={ix["wood"]: 1, ix["iron"]: 1, ix["plank"]: 2, ix["stick"]: 1, ix["grass"]: 1}, script=s)]
    return _case(recipes, grid, rows)


def _scatter():
    """The scatter over four lanes per env: agents in the four corners of the interior, on its
    four edges and in the middle, so that the 9x9 pooled window is clipped on every side (and on
    two at once), facing every direction, with an inventory of many kinds, on a grid about a third
    full of every kind; random actions (USE often, STOP seldom) move them about.  A block row
    scattered by the wrong lane, or twice, or not at all, changes the observation."""
    ix, tm, grid, K = _base()
    rng = np.random.RandomState(7)
    starts = [(1, 1), (1, 10), (10, 1), (10, 10), (1, 5), (10, 5), (5, 1), (5, 10), (5, 5)]
    kinds = [ix[k] for k in ("wood", "iron", "grass", "gold", "gem", "water", "stone", "workshop0", "workshop1", "workshop2")]
    for x in range(1, W - 1):
        for y in range(1, W - 1):
            if (x, y) not in starts and rng.rand() < 0.35:
                grid[x, y] = kinds[rng.randint(len(kinds))]
    tasks = [t.id for t in tm.dataset_tasks()]
    c = _case(None, grid, [lambda j, p=p: dict(x=p[0], y=p[1], dir=j % 4, task=tasks[(j + p[0]) % len(tasks)],
                                               inv={k: (j + k) % 4 for k in range(7, K)}, script=[STOP])
                           for p in starts])
    c["acts"] = rng.choice(6, size=(T, NMAX), p=[.17, .17, .17, .17, .28, .04]).astype(np.int32)
    return c


_BUILDERS = {"neighbours": _neighbours, "inventory": lambda: _inventory(True), "freeze": lambda: _inventory(False),
             "chained": lambda: _recipes(chained_recipes()), "generic": lambda: _recipes(triple_recipes()),
             "scatter": _scatter}
_cases, _refs = {}, {}
_MARKS = (5, 6, 15, 30)                                  # the split launches' ends


def _outputs(sim, rows, dev, dtype=torch.float32):
    n = sim.n_envs
    return {"obs": torch.zeros((rows, n, sim.n_features), dtype=dtype, device=dev),
            "reward": torch.zeros((rows, n), dtype=torch.float32, device=dev),
            "done": torch.zeros((rows, n), dtype=torch.uint8, device=dev),
            "success": torch.zeros((rows, n), dtype=torch.int8, device=dev)}


def _state(sim):
    return {k: t.cpu().numpy() for k, t in sim.get_state().items()}


def _check_scripts(name, case, ref, n):
    """The reference does what the scripts' docstrings say (so that a mis-built scenario cannot
    pass on both sides): per env type, positions, cells, counts and successes at chosen ticks.
    ref["agent"][t] is the agent after tick t, ref["states"][m] the state after m ticks."""
    sim = CraftSim(WORLD, n_envs=1, device="cpu", pool_capacity=1, recipes=case["recipes"])
    ix = sim.cookbook.index
    ag, succ, done, st = ref["agent"], ref["success"], ref["done"], ref["states"]
    cell = lambda m, i, x, y: int(st[m]["grid"][i, x * W + y])      # noqa: E731
    inv = lambda m, i, k: int(st[m]["inventory"][i, ix[k]])          # noqa: E731
    for i in range(n):
        ty, j = i % 5, i // 5
        if name == "neighbours":
            if ty in (0, 1, 2):
                assert ag[2, i, 0] == 3, (i, "walks through the cell it cleared")
                assert ag[6, i, 0] == 1 and cell(6, i, 2, 1 + 2 * ty) != 0, (i, "blocked by the restored cell")
            if ty == 0:
                assert cell(15, i, 2, 1) == 0 and inv(15, i, "wood") == 1, (i, "grabbed again")
            if ty in (1, 2):
                assert cell(15, i, 2, 1 + 2 * ty) != 0 and st[15]["inventory"][i].sum() == 0, (i, "nothing to clear with")
            if ty == 3:
                assert succ[3, i] == (1 if j % 2 == 0 else 0), (i, "go[wood] facing the wood, get[wood] without any")
                assert ag[6, i, 1] == 8 and inv(15, i, "wood") == 1, (i, "walks into the cell it grabbed from")
            if ty == 4:
                assert ag[9, i, 0] == 6 and done[10, i] == 1 and ag[11, i, 0] == 1, (i, "five clears, restart, blocked")
                assert [cell(15, i, x, 9) for x in range(2, 8)] == [0, 0] + [ix["wood"]] * 4, (i, "whole row restored")
        elif name in ("inventory", "freeze"):
            frozen = name == "freeze"
            if ty == 0:
                assert [inv(5, i, k) for k in ("wood", "iron", "grass")] == [1, 1, 1] and succ[10, i] == 1, i
                assert inv(15, i, "grass") == (1 if frozen else 0) and inv(15, i, "wood") == (2 if frozen else 1), i
                if frozen:
                    assert done[10:, i].all() and (ag[10, i] == ag[T - 1, i]).all(), i
            if ty == 1:
                assert succ[1, i] == 1 and succ[2, i] == (1 if frozen else 0), (i, "success follows the count")
                assert not frozen or (done[1:, i].all() and (succ[1:, i] == 1).all()), i
            if ty == 2:
                assert succ[1, i] == 1 and succ[3, i] == (1 if frozen else 0), (i, "made, then nothing to make from")
            if ty == 3 and not frozen:
                assert ag[1, i, 0] == 2 and succ[3, i] == 1 and inv(5, i, "iron") == 1, (i, "grabbed, and again after the restart")
            if ty == 4:
                assert (st[5]["inventory"][i, 7:sim.n_kinds] > 0).all(), (i, "the row carried unchanged")
        elif name in ("chained", "generic"):
            assert done[6, i] == 1 and st[15]["inventory"][i].sum() == 0, (i, "restart empties the inventory")
            if ty == 0:
                assert inv(5, i, "rope") == 3 and inv(5, i, "axe") == (1 if name == "chained" else 0), i
                assert succ[6, i] == (1 if name == "chained" else 0), i
            if ty == 1:
                assert inv(5, i, "plank") == 1 and inv(5, i, "axe") == 0 and succ[6, i] == 1, i
            if ty == 2:
                assert inv(5, i, "shears") >= 1 and inv(5, i, "bed") == 1, (i, "bed from two or three ingredients")
            if ty == 3:
                assert st[5]["inventory"][i].sum() == 0 and succ[6, i] == 0, (i, "every USE lacks its ingredients")
            if ty == 4:
                assert inv(5, i, "bridge") == 1 and inv(5, i, "ladder") == 1 and inv(5, i, "cloth") == 1, i
        else:
            assert (ref["obs"][:, i] != 0).sum(-1).min() > 9, (i, "an observation with pooled cells")


def _reference(name, n):
    """The case's 30 ticks on its first n envs: the CPU variant's one rollout and a GPU twin's 30
    craft_step calls (with its state after ticks 5, 6, 15 and 30), equal to each other; computed
    once per (case, n) and left unchanged."""
    if (name, n) in _refs:
        return _cases[name], _refs[(name, n)]
    case = _cases.setdefault(name, _BUILDERS[name]())
    acts = np.ascontiguousarray(case["acts"][:, :n])
    cpu = _sim(case, n, "cpu")
    _start(cpu, case, n)
    out = _outputs(cpu, T, "cpu")
    cpu.rollout(T, actions=torch.as_tensor(acts), autoreset=case["autoreset"], **out)
    cpu.check()
    ref = {k: t.numpy() for k, t in out.items()}
    ref["stats"] = cpu.stats().numpy()
    ref_state = _state(cpu)
    twin = _sim(case, n, 0)
    _start(twin, case, n)
    out = _outputs(twin, T, "cuda")
    dacts = torch.as_tensor(acts, device="cuda")
    states, agents = {}, []
    for t in range(T):
        twin.step(dacts[t], tick=t, autoreset=case["autoreset"], obs=out["obs"][t], reward=out["reward"][t],
                  done=out["done"][t], success=out["success"][t])
        agents.append(twin.get_state(fields=("agent",))["agent"].cpu().numpy())
        if t + 1 in _MARKS:
            states[t + 1] = _state(twin)
    twin.check()
    for k, t in out.items():
        np.testing.assert_array_equal(t.cpu().numpy(), ref[k], err_msg=f"{name}: steps vs cpu {k}")
    for k, v in ref_state.items():
        np.testing.assert_array_equal(states[T][k], v, err_msg=f"{name}: steps vs cpu state {k}")
    np.testing.assert_array_equal(twin.stats().cpu().numpy(), ref["stats"])
    ref["states"], ref["agent"] = states, np.stack(agents)
    # not vacuous: episodes end, steps are counted, and every script does what its docstring says
    assert ref["done"].any() and ref["stats"][2] > 0
    _check_scripts(name, case, ref, n)
    _refs[(name, n)] = ref
    return case, ref


def _run(name, n, shape, fmt="f32"):
    case, ref = _reference(name, n)
    acts = torch.as_tensor(np.ascontiguousarray(case["acts"][:, :n]), device="cuda")
    for launches in LAUNCHES:
        for ring in RINGS:
            what = f"{name} n={n} {shape} launches={launches} ring={ring} {fmt}"
            sim = _sim(case, n, 0)
            if SHAPES[shape] is not None:
                tile, threads, chunk = SHAPES[shape]
                sim.tune(tile, 0, 0)
                sim.tune_rollout(chunk, threads)
            sim.set_obs_format(fmt)
            _start(sim, case, n)
            out = _outputs(sim, ring, "cuda", sim.obs_dtype)
            t0 = 0
            for K in launches:
                sim.rollout(K, tick0=t0, actions=acts[t0:t0 + K], autoreset=case["autoreset"], **out)
                t0 += K
                for r in range(min(ring, t0)):           # slot r holds the last tick t < t0 with t % ring == r
                    t = r + (t0 - 1 - r) // ring * ring
                    for k, x in out.items():
                        np.testing.assert_array_equal(x[r].float().cpu().numpy(), ref[k][t].astype(np.float32),
                                                      err_msg=f"{what}: {k} of tick {t}")
                for k, v in _state(sim).items():
                    np.testing.assert_array_equal(v, ref["states"][t0][k], err_msg=f"{what}: state {k} after tick {t0}")
            np.testing.assert_array_equal(sim.stats().cpu().numpy(), ref["stats"], err_msg=what)
            sim.check()


_SIZES = (1, 33, 70)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", _SIZES)
def test_carried_neighbour_kinds(n, shape):
    """The kinds around the agent after a tick are the next tick's facing cell and move target,
    read from the other parity buffer.  Stale after a USE that cleared the facing cell: the walk into it is blocked.  Stale
    after a restart: the agent, back at its start, walks through restored wood, water or stone, or
    grabs from an empty cell.  A cleared cell's remembered kind wrong: the restart restores another
    kind, or nothing, which the next observation and get_state() show; past three clears the
    whole row must come back.  (_neighbours has the scripts.)"""
    _run("neighbours", n, shape)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", _SIZES)
@pytest.mark.parametrize("case", ["inventory", "freeze"])
def test_inventory_row_across_ticks(case, n, shape):
    """The inventory row after a tick is carried into the next tick's buffer and answers
    satisfies().  Stale by a tick: a get / make task's success on the tick after the count changed
    is missed.  Stale across a restart: the new episode starts with the old counts, its first STOP
    succeeds, and its observations show them.  Frozen (no auto-reset): the row must keep being
    written to both buffers unchanged.  (_inventory has the scripts.)"""
    _run(case, n, shape)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", _SIZES)
@pytest.mark.parametrize("case", ["chained", "generic"])
def test_workshop_recipe_table(case, n, shape):
    """A workshop's USE inside a K-tick launch (chained: a product that is the next recipe's
    ingredient, an output that is its own ingredient, a USE that lacks one ingredient; generic: a
    cookbook with a three-ingredient recipe, which no compact per-workshop table holds).  Recipes
    run for the wrong workshop, or out of order, craft the wrong things; the inventory carried to
    the next tick must also pick up what the USE wrote.  (_recipes has the scripts.)"""
    _run(case, n, shape)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("fmt,n", [("f32", 1), ("f32", 33), ("f32", 70), ("bf16", 2), ("bf16", 34), ("bf16", 70),
                                   ("u8", 4), ("u8", 36), ("u8", 72)])
def test_scatter_lanes(fmt, n, shape):
    """Observations with the scatter on four lanes per env (32-env tiles) or as before (16-env
    tiles), in every observation format: clipped windows on each side, every direction, many
    inventory kinds.  craft_rollout takes an observation ring only if every slot is 16-byte
    aligned (n * 404 elements here), so bf16 runs the nearest even sizes (2, 34, 70) and u8 the
    nearest multiples of four (4, 36, 72) instead of 1, 33 and 70: still the smallest tile, a
    few envs past a 32-env tile, and full tiles with a partial one.  (_scatter has the layout.)"""
    _run("scatter", n, shape, fmt)
