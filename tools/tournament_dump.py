"""What the tournament driver computes, as text that two commits can be compared by: one JSON line per cell of
tests/test_gpu_tournament_engines.py's table (engine, wins, avg_length and the sha256 of the scores' and the lengths' bytes; for a
chunked cell also with chunk=3 and, where it has one, on the per-step loop), then the rows of three CLI tables with the same fields and
the sha256 of everything the CLI printed.

    python tools/tournament_dump.py CHECKPOINT

CHECKPOINT: a 5x5 checkpoint of any of the trainers (trainer.save).  Run it in a fresh process per commit, on the same checkpoint."""
import contextlib
import hashlib
import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ewn_gym_amd import tournament  # noqa: E402
from tests.test_gpu_tournament_engines import CHUNKED, NONE, cells, play  # noqa: E402


def digest(r):
    sha = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()   # noqa: E731
    return {"engine": r["engine"], "wins": r["wins"], "avg_length": r["avg_length"], "scores": sha(r["scores"]), "lengths": sha(r["lengths"])}


def cli(ckpt, argv):
    """tournament.main() under argv: its table's rows with the digests of the evaluations behind them, and its output's sha256"""
    played = []
    saved = tournament.evaluate, tournament.evaluate_vs_model

    def recording(fn):
        def call(*args, **kw):
            played.append(fn(*args, **kw))
            return played[-1]
        return call
    out = io.StringIO()
    tournament.evaluate, tournament.evaluate_vs_model = recording(saved[0]), recording(saved[1])
    sys.argv = ["tournament"] + argv
    try:
        with contextlib.redirect_stdout(out):
            tournament.main()
    finally:
        tournament.evaluate, tournament.evaluate_vs_model = saved
    rows = json.loads(out.getvalue().strip().splitlines()[-1])
    assert len(rows) == len(played), (list(rows), len(played))    # one evaluation per row, in the table's order
    name = " ".join("CKPT" if x == ckpt else x for x in argv)       # the same line wherever the checkpoint lies
    for (label, row), r in zip(rows.items(), played):
        d = digest(r)
        assert (row["engine"], row["wins"], row["avg_length"]) == (d["engine"], d["wins"], d["avg_length"]), label
        print(json.dumps({"cli": name, "row": label, **d}), flush=True)
    print(json.dumps({"cli": name, "stdout": hashlib.sha256(out.getvalue().encode()).hexdigest()}), flush=True)


def main():
    ckpt = sys.argv[1]
    model = tournament.load_policy(ckpt)
    for cell in cells(model, lambda b, d, t: model.act(b, d, deterministic=True)[0]):
        line = {"cell": cell[0], **digest(play(cell))}
        if cell[5] in CHUNKED:
            line["chunk=3"] = digest(play(cell, use_rollout=True, chunk=3))
            if cell[6] is not NONE:
                line["use_rollout=False"] = digest(play(cell, use_rollout=False))
        print(json.dumps(line), flush=True)
    common = ["--agents", "random", "minimax", "--num", "64", "--max_depth", "3"]
    cli(ckpt, common)
    cli(ckpt, ["--model", ckpt] + common + ["--lookahead", "--puct", "8"])
    cli(ckpt, ["--opponent_model", ckpt] + common)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
