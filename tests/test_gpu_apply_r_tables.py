"""gpu: what apply_r.main takes from Context.malloc it gives back by the time it returns - on every route, and when a step in the middle of
the run raises.  Context.malloc and Context.free are wrapped (upload goes through malloc) and the pointers counted; the failures are plain
Python exceptions raised on entry of a replaced step, nothing is made to fail on the GPU.  Smallest corpus throughout: the similarity search
needs 500 rows, SSIM's window 11 pixels."""
import pytest

from test_gpu_apply_r_dataset import DATASET, folder      # noqa: F401  (fixtures: 520 tiny .npy images under tmp_path; ganrev.dataset put back)

pytestmark = pytest.mark.gpu

BASE = ["--synthetic", "1x32x32x32", "--nbImages", "600", "--batchSize", "64", "--quiet", "--nbIterations", "2"]
MAP = ["--map", "--mapRows", "64", "--mapPerplexity", "5", "--mapIterations", "20", "--mapGrid", "4"]
EVERYTHING = ["--resident", "--pca", "4", "--pcaSpace"] + MAP + ["--mixture", "2", "--refine", "2", "--anomalyMetric", "ssim"]
ROUTES = {"host": ["--host"], "host-render": ["--host", "--render"], "device": [], "render": ["--render"], "resident": ["--resident"],
          "resident-everything": EVERYTHING}
# nothing the package allocates through Context.malloc during a run is kept for the life of the process: the compiled nets, the dataset cache
# and the library's scratch buffers are the C side's own and do not come from here.  So the rule has no exception: no pointer is left.


@pytest.fixture
def ledger(monkeypatch):
    """pointer -> bytes of everything Context.malloc handed out and Context.free has not taken back"""
    import ganrev._lib as L
    live, handed = {}, []
    malloc, free = L.Context.malloc, L.Context.free

    def counting_malloc(self, nbytes):
        p = malloc(self, nbytes)
        live[p] = int(nbytes)
        handed.append(p)
        return p

    def counting_free(self, p):
        free(self, p)
        live.pop(getattr(p, "value", p), None)
    monkeypatch.setattr(L.Context, "malloc", counting_malloc)
    monkeypatch.setattr(L.Context, "free", counting_free)
    return live, handed


def leftovers(ledger):
    live, handed = ledger
    assert handed, "the run took its tables from Context.malloc: the wrappers saw it"
    return {hex(p): n for p, n in live.items()}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_table_of_a_run_is_freed(tmp_path, ledger, route):
    from ganrev import apply_r
    summary = apply_r.main(BASE + ROUTES[route] + ["--writeTo", str(tmp_path / route)])
    assert summary["nbImages"] == 600 and "anomalies" in summary
    assert leftovers(ledger) == {}


FAILING = {"pca.principalAxes": EVERYTHING, "tsne.embed": EVERYTHING, "mixture.fit": EVERYTHING, "refine.refineNoise": EVERYTHING,
           "apply_r.createSimilaritySearchDev": EVERYTHING, "apply_r.createClusterImagesDev": EVERYTHING, "render.variations_grid": ["--render"]}


@pytest.mark.parametrize("step", sorted(FAILING))
def test_every_table_is_freed_when_a_step_raises(tmp_path, monkeypatch, ledger, step):
    import importlib
    from ganrev import apply_r
    from ganrev._lib import GanrevError

    def broken(*args, **kwargs):
        raise GanrevError("broken on purpose: " + step)
    module, name = step.split(".")
    monkeypatch.setattr(importlib.import_module("ganrev." + module), name, broken)
    with pytest.raises(GanrevError, match="broken on purpose: " + step):
        apply_r.main(BASE + FAILING[step] + ["--writeTo", str(tmp_path / "out")])
    assert leftovers(ledger) == {}


@pytest.mark.parametrize("fails", [False, True], ids=["runs", "search-raises"])
@pytest.mark.parametrize("flags", [["--needles", "2"], ["--real", "--resident"]], ids=["needles", "real"])
def test_dataset_runs_free_their_tables_and_the_cache(tmp_path, monkeypatch, ledger, folder, DATASET, flags, fails):
    from ganrev import apply_r
    from ganrev._lib import GanrevError

    def broken(*args, **kwargs):
        raise GanrevError("broken on purpose: searchByExample")
    args = BASE + flags + ["--dataset", folder, "--fileExtension", "npy", "--cacheDataset", "--writeTo", str(tmp_path / "out")]
    if "--real" in flags:
        args[args.index("--nbImages") + 1] = "520"                                         # the corpus is the folder's 520 files
    if fails:
        monkeypatch.setattr(apply_r, "searchByExample", broken)
        with pytest.raises(GanrevError, match="broken on purpose"):
            apply_r.main(args + ([] if "--needles" in flags else ["--needles", "2"]))      # (--real alone never searches by example)
    else:
        assert ("needles" in apply_r.main(args)) == ("--needles" in flags)
    assert leftovers(ledger) == {}
    assert not DATASET.cached(), "dataset.uncache() has run"
