"""Writes tests/golden/post_golden.json: what the reference's own post-processor returns on the clips of tests/post_cases.py.

    python tests/golden/make_post_golden.py <path of the reference checkout> [--check]

Needs pandas and scikit-learn (imports of the reference's eagle/processor.py); cv2 is replaced by a stub whose only working part is
KalmanFilter.predict, the documented assumption of tests/post_ref.py::kalman_predict.  ``get_team_mapping`` is stubbed to return the case's mapping
(team colours have their own golden).  Only data leaves this script: per case the clip as tests/post_cases.py states it (so a change of the cases
shows), and per ``smooth`` value the table (kept frame numbers, column names, cells as JSON numbers, which round-trip float64 exactly; missing =
null) and the rows of ``format_data`` — runs of [count, [boundary columns, items, video items]] with an item = [ID, Type | null, column]: this script
checks that every value format_data emits IS the table cell of that column, so the reference into the table loses nothing — or the name of the
exception the reference raises.  One JSON line per case and ``smooth`` value.  --check compares with the committed file instead."""
import importlib.util
import json
import math
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import post_cases  # noqa: E402
import post_ref  # noqa: E402

OUT = os.path.join(HERE, "post_golden.json")


class _StubKalman:
    def __init__(self, dynam, measure):
        self.statePre = np.zeros((dynam, 1), np.float32)
        self.statePost = np.zeros((dynam, 1), np.float32)

    def predict(self):
        self.statePre, self.statePost = post_ref.kalman_predict(self.statePost)
        return self.statePre

    def correct(self, measurement):
        raise NotImplementedError("cv2.KalmanFilter.correct is not restated (filter_ball_detections=True is out of scope)")


def load_reference(root):
    cv2 = types.ModuleType("cv2")
    cv2.KalmanFilter = _StubKalman
    sys.modules["cv2"] = cv2
    spec = importlib.util.spec_from_file_location("reference_processor", os.path.join(root, "eagle", "processor.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _num(v):
    v = float(v)
    return None if math.isnan(v) else v


def _cell(v):
    if isinstance(v, (tuple, list)):
        return [_num(v[0]), _num(v[1])]
    assert v is None or (isinstance(v, float) and math.isnan(v)), repr(v)
    return None


def run_case(ref, case, smooth):
    coords = post_cases.coords_of(case)
    frames = [np.zeros((2, case["frame_w"], 3), np.uint8)] * len(coords)
    try:
        proc = ref.Processor(coords, frames, case["fps"], filter_ball_detections=False)
        proc.get_team_mapping = lambda: dict(case["team_mapping"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            df, team_mapping = proc.process_data(smooth=smooth)
            fmt = proc.format_data(df) if not df.empty else None
    except Exception as e:      # noqa: BLE001  (the name of what the reference raises is the recorded result)
        return {"raises": type(e).__name__}
    out = {"rows": [int(i) for i in df.index], "columns": [str(c) for c in df.columns],
           "values": [[_cell(v) for v in df[c]] for c in df.columns], "team_mapping": {str(k): int(v) for k, v in team_mapping.items()}}
    cols = list(df.columns)

    def column_of(val, frame_number, candidates):
        """the column whose cell in this row format_data handed out as `val`"""
        for c in candidates:
            cur = df.loc[frame_number, cols[c]]
            if cur is val or (_cell(cur) is None and _cell(val) is None):
                assert _cell(cur) == _cell(val)
                return c
        raise AssertionError(f"format_data value {val!r} is no cell of row {frame_number}")

    out["format"] = []
    for frame_number, row in zip(df.index, [] if fmt is None else fmt.to_dict("records")):
        assert list(row) == ["Boundaries", "Coordinates", "Coordinates_video"]
        bounds = [column_of(b, frame_number, [cols.index(n)]) for b, n in zip(row["Boundaries"], post_ref.BOUNDARIES)]
        lists = []
        for key, ball in (("Coordinates", "Ball"), ("Coordinates_video", "Ball_video")):
            items = []
            for it in row[key]:
                assert sorted(it) in (["Coordinates", "ID"], ["Coordinates", "ID", "Type"])
                cand = [cols.index(ball)] if it["ID"] == "Ball" else [c for c, n in enumerate(cols) if "Ball" not in n and n not in post_ref.BOUNDARIES]
                items.append([it["ID"], it.get("Type"), column_of(it["Coordinates"], frame_number, cand)])
            lists.append(items)
        row = [bounds] + lists
        if out["format"] and out["format"][-1][1] == row:
            out["format"][-1][0] += 1                   # run-length: [count, row] for consecutive rows of one shape
        else:
            out["format"].append([1, row])
    return out


def build(root):
    import pandas
    ref = load_reference(root)
    cases = {}
    for case in post_cases.CASES:
        sys.stdout = open(os.devnull, "w")          # the reference prints
        try:
            res = {f"smooth{int(s)}": run_case(ref, case, s) for s in (False, True)}
        finally:
            sys.stdout = sys.__stdout__
        cases[case["name"]] = dict(clip={"fps": case["fps"], "frame_w": case["frame_w"], "team_mapping": {str(k): v for k, v in case["team_mapping"].items()},
                                         "frames": json.loads(json.dumps(case["frames"]))}, **res)
    return {"pandas": pandas.__version__, "cases": cases}


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    g = build(argv[1])
    dump = lambda o: json.dumps(o, separators=(",", ":"), allow_nan=False)      # noqa: E731
    lines = []
    for name, c in g["cases"].items():
        lines.append(f'{dump(name)}:{{"clip":{dump(c["clip"])},\n"smooth0":{dump(c["smooth0"])},\n"smooth1":{dump(c["smooth1"])}}}')
    text = f'{{"pandas":{dump(g["pandas"])},"cases":{{\n' + ",\n".join(lines) + "\n}}\n"
    assert json.loads(text) == g
    if "--check" in argv[2:]:
        same = open(OUT).read() == text
        print("post_golden.json", "matches" if same else "DIFFERS from what the reference returns now")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print(f"{OUT}: {len(text)} bytes, {len(post_cases.CASES)} cases")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv))
