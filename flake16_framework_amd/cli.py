"""Command-line interface — compatible with the reference's
`python experiment.py COMMAND` surface (experiment.py:693-714) plus
GPU/synthetic extensions:

  setup                      provision subject venvs (docker build time)
  container NAME CMD...      in-container runner
  run MODE...                data collection (baseline/shuffle/testinspect)
  tests                      collate data/ -> tests.json
  scores                     216-cell grid -> scores.pkl (GPU when present)
  shap                       TreeSHAP for the 2 best configs -> shap.pkl
  figures                    LaTeX tables/plots

  synthetic [--n-tests N] [--seed S]   write a synthetic tests.json
  scores/shap extras: --backend {auto,hip,ref}

  fit [--config nod|od] [--keys K0 K1 K2 K3 K4] [--backend B]
      [--tests-file F] [--detector OUT] [--n-trees N]
                             fit one configuration on tests.json and save
                             it -> detector.npz.  nod / od are the study's
                             two best configurations (configgrid
                             SHAP_CONFIGS); --keys names any grid cell by
                             its five display keys
  detect [--detector F] [--tests-file F] [--out F] [--backend B]
                             apply a saved detector to a tests.json ->
                             detections.json {proj: {nodeid: [proba, pred]}}
  explain [--detector F] [--tests-file F] [--out F] [--backend B]
                             detect plus TreeSHAP: split every test's
                             flaky-class probability into one contribution
                             per model input -> explanations.json
                             {"feature_names", "base_value", "tests":
                             {proj: {nodeid: [proba, pred, phi...]}}};
                             class-1 values, the negation of shap.pkl's
  interact [--detector F] [--tests-file F] [--out F] [--top N]
      [--matrix-out F] [--backend B]
                             explain plus SHAP interaction values: every
                             test's probability split into an [F, F]
                             matrix whose row g sums to phi[g] ->
                             interactions.json {"feature_names",
                             "base_value", "mean_abs", "pairs", "tests":
                             {proj: {nodeid: [proba, pred, [diagonal],
                             [[g, f, Phi[g,f] + Phi[f,g]], ...]]}}} with
                             the N (default 3) strongest pairs per test;
                             --matrix-out saves the full [M, F, F] array
                             as .npy
  holdout[--config nod|od] [--keys K0 K1 K2 K3 K4] [--backend B]
      [--tests-file F] [--out F] [--n-trees N] [--thresholds K]
      [--detections F]
                             leave-one-project-out evaluation: every
                             project is classified by a detector fitted on
                             the other projects only -> holdout.json with
                             per-project and pooled [FP, FN, TP] under the
                             argmax rule and under proba >= k / (K - 1);
                             --detections also writes the out-of-fold
                             {proj: {nodeid: [proba, pred]}}
  importance [--detector F] [--tests-file F] [--out F] [--repeats R]
      [--seed S] [--threshold T] [--backend B]
      [--holdout [--config nod|od | --keys K0 K1 K2 K3 K4] [--n-trees N]]
                             permutation importance on a labelled
                             tests.json: each raw feature, and each of the
                             families Coverage / Resource Usage / Static,
                             is permuted inside every project R times and
                             the tests are classified again ->
                             importance.json with the baseline and per
                             group the pooled and per-project [FP, FN, TP]
                             and the mean drop in F1 and recall.  The rule
                             is argmax, or proba >= T with --threshold.
                             --holdout fits one detector per held-out
                             project first (as `holdout` does) and scores
                             every project with the detector that never
                             saw it
  similar [--detector F] [--tests-file F] [--corpus F] [--out F] [--k K]
      [--flaky-only] [--keep-self] [--backend B]
                             forest proximity: for every test of the
                             tests file the K (1..16, default 5) tests of
                             the labelled corpus (default tests.json) that
                             share a leaf with it in the most trees, ties
                             to the earlier corpus test -> similar.json
                             {"k", "n_trees", "corpus_tests", "tests":
                             {proj: {nodeid: [proba, pred, [[corpus_proj,
                             corpus_nodeid, label, shared], ...]]}}}.
                             --flaky-only ranks the flaky corpus tests
                             only; a test found in the corpus under its
                             own (project, nodeid) is left out unless
                             --keep-self is given
  dependence [--detector F] [--tests-file F] [--out F] [--grid V]
      [--threshold T] [--ice-out F.npy] [--backend B]
                             partial dependence: every raw feature of the
                             detector is set, in all tests at once, to
                             each of up to V (2..64, default 20) values
                             between its 5th and 95th percentile, and the
                             tests are classified again ->
                             dependence.json {"config_keys", "rule",
                             "threshold", "n_tests", "baseline", "features":
                             {name: {"grid", "mean_proba", "flagged",
                             "range", "projects": {proj: {"mean_proba",
                             "flagged"}}}}}: the mean flaky probability
                             and the number of tests predicted flaky
                             (argmax, or proba >= T with --threshold) at
                             every grid value, pooled and per project.
                             --ice-out saves the per-test curves as a
                             float64 [tests, jobs] .npy

Distributed: launch via `python -m torch.distributed.run --nproc-per-node N
experiment.py scores` — one rank per GPU over RCCL; rank 0 writes the
artifacts.
"""

import sys


def _pop_flag(args, name, default=None, boolean=False):
    if name in args:
        i = args.index(name)
        if boolean:
            args.pop(i)
            return True
        args.pop(i)
        return args.pop(i)
    return default


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv:
        raise ValueError("No command given")

    command, *args = argv

    if command == "setup":
        from .orchestrate.runner import provision_all
        provision_all()
    elif command == "container":
        from .orchestrate.runner import exec_suite
        exec_suite(*args)
    elif command == "run":
        from .orchestrate.runner import drive_runs
        drive_runs(*args)
    elif command == "tests":
        from .dataset.tests_io import write_tests
        write_tests()
    elif command == "scores":
        backend = _pop_flag(args, "--backend", "auto")
        checkpoint = _pop_flag(args, "--checkpoint", None)
        n_cells = _pop_flag(args, "--cells", None)
        trace = _pop_flag(args, "--trace", None)
        if trace:
            from .utils.trace import set_trace_file
            set_trace_file(trace)
        from .engine.scores import write_scores
        from .parallel import comm
        comm.init_from_env()
        write_scores(backend=backend, checkpoint=checkpoint,
                     n_cells=int(n_cells) if n_cells else None)
    elif command == "shap":
        backend = _pop_flag(args, "--backend", "auto")
        from .engine.shap_stage import write_shap
        from .parallel import comm
        comm.init_from_env()
        write_shap(backend=backend)
    elif command == "fit":
        from .configgrid import SHAP_CONFIGS
        from .constants import DETECTOR_FILE, TESTS_FILE
        from .engine.detector import fit_detector
        config = _pop_flag(args, "--config", "nod")
        if config not in ("nod", "od"):
            raise ValueError("--config takes nod or od")
        keys = SHAP_CONFIGS[("nod", "od").index(config)]
        if "--keys" in args:
            i = args.index("--keys")
            keys = tuple(args[i + 1:i + 6])
            if len(keys) != 5:
                raise ValueError("--keys takes five config keys")
            del args[i:i + 6]
        backend = _pop_flag(args, "--backend", "auto")
        tests_file = _pop_flag(args, "--tests-file", TESTS_FILE)
        out = _pop_flag(args, "--detector", DETECTOR_FILE)
        n_trees = _pop_flag(args, "--n-trees", None)
        det = fit_detector(keys, tests_file=tests_file, backend=backend,
                           n_trees=int(n_trees) if n_trees else None)
        det.save(out)
        print(f"wrote {out} ({' / '.join(det.config_keys)}, "
              f"{det.n_trees} trees, {det.n_train} training tests)")
    elif command == "detect":
        from .constants import DETECTIONS_FILE, DETECTOR_FILE, TESTS_FILE
        from .engine.detector import Detector, write_detections
        detector_file = _pop_flag(args, "--detector", DETECTOR_FILE)
        tests_file = _pop_flag(args, "--tests-file", TESTS_FILE)
        out = _pop_flag(args, "--out", DETECTIONS_FILE)
        backend = _pop_flag(args, "--backend", "auto")
        res = write_detections(Detector.load(detector_file),
                               tests_file=tests_file, out_file=out,
                               backend=backend)
        print(f"wrote {out} ({len(res['pred'])} tests, "
              f"{int(res['pred'].sum())} predicted flaky)")
    elif command == "explain":
        import numpy as np
        from .constants import DETECTOR_FILE, EXPLANATIONS_FILE, TESTS_FILE
        from .engine.detector import Detector
        from .engine.explain import write_explanations
        detector_file = _pop_flag(args, "--detector", DETECTOR_FILE)
        tests_file = _pop_flag(args, "--tests-file", TESTS_FILE)
        out = _pop_flag(args, "--out", EXPLANATIONS_FILE)
        backend = _pop_flag(args, "--backend", "auto")
        res = write_explanations(Detector.load(detector_file),
                                 tests_file=tests_file, out_file=out,
                                 backend=backend)
        weight = np.abs(res["phi"]).sum(axis=0) / max(1, len(res["phi"]))
        top = ", ".join(f"{res['feature_names'][f]} {weight[f]:.4f}"
                        for f in np.argsort(-weight, kind="stable")[:3])
        print(f"wrote {out} ({len(res['pred'])} tests; "
              f"largest mean |phi|: {top})")
    elif command == "interact":
        from .constants import DETECTOR_FILE, INTERACTIONS_FILE, TESTS_FILE
        from .engine.detector import Detector
        from .engine.interact import (
            pair_index, rank_pairs, summarize, write_interactions,
        )
        detector_file = _pop_flag(args, "--detector", DETECTOR_FILE)
        tests_file = _pop_flag(args, "--tests-file", TESTS_FILE)
        out = _pop_flag(args, "--out", INTERACTIONS_FILE)
        top = int(_pop_flag(args, "--top", "3"))
        matrix_out = _pop_flag(args, "--matrix-out", None)
        backend = _pop_flag(args, "--backend", "auto")
        res = write_interactions(Detector.load(detector_file),
                                 tests_file=tests_file, out_file=out,
                                 top=top, matrix_out=matrix_out,
                                 backend=backend)
        names = res["feature_names"]
        pairs = pair_index(len(names))
        _, weight = summarize(res["interactions"])
        best = ", ".join(
            f"{names[pairs[p, 0]]} x {names[pairs[p, 1]]} {weight[p]:.4f}"
            for p in rank_pairs(weight)[:3])
        print(f"wrote {out} ({len(res['pred'])} tests; "
              f"largest mean |Phi[g,f] + Phi[f,g]|: {best})")
    elif command == "holdout":
        from .configgrid import SHAP_CONFIGS
        from .constants import HOLDOUT_FILE, TESTS_FILE
        from .engine.holdout import best_f1_threshold, write_holdout
        config = _pop_flag(args, "--config", "nod")
        if config not in ("nod", "od"):
            raise ValueError("--config takes nod or od")
        keys = SHAP_CONFIGS[("nod", "od").index(config)]
        if "--keys" in args:
            i = args.index("--keys")
            keys = tuple(args[i + 1:i + 6])
            if len(keys) != 5:
                raise ValueError("--keys takes five config keys")
            del args[i:i + 6]
        backend = _pop_flag(args, "--backend", "auto")
        tests_file = _pop_flag(args, "--tests-file", TESTS_FILE)
        out = _pop_flag(args, "--out", HOLDOUT_FILE)
        n_trees = _pop_flag(args, "--n-trees", None)
        n_thresholds = int(_pop_flag(args, "--thresholds", "101"))
        detections = _pop_flag(args, "--detections", None)
        res = write_holdout(keys, tests_file=tests_file, out_file=out,
                            detections_file=detections, backend=backend,
                            n_trees=int(n_trees) if n_trees else None,
                            n_thresholds=n_thresholds)
        fmt = lambda v: "n/a" if v is None else f"{v:.4f}"
        p, r, f = res["total"]["argmax"][3:]
        best = best_f1_threshold(res["total"]["curve"], res["thresholds"])
        best = ("none" if best is None
                else f"{best[1]:.4f} (F1 {best[2]:.4f}, descriptive)")
        print(f"wrote {out} ({len(res['projects'])} held-out projects, "
              f"{res['n_trees']} trees; pooled argmax P {fmt(p)} "
              f"R {fmt(r)} F1 {fmt(f)}; best-F1 threshold {best})")
    elif command == "importance":
        from .configgrid import SHAP_CONFIGS
        from .constants import DETECTOR_FILE, IMPORTANCE_FILE, TESTS_FILE
        from .engine.importance import holdout_importance, write_importance
        leave_out = _pop_flag(args, "--holdout", False, boolean=True)
        config = _pop_flag(args, "--config", "nod")
        if config not in ("nod", "od"):
            raise ValueError("--config takes nod or od")
        keys = SHAP_CONFIGS[("nod", "od").index(config)]
        if "--keys" in args:
            i = args.index("--keys")
            keys = tuple(args[i + 1:i + 6])
            if len(keys) != 5:
                raise ValueError("--keys takes five config keys")
            del args[i:i + 6]
        detector_file = _pop_flag(args, "--detector", DETECTOR_FILE)
        tests_file = _pop_flag(args, "--tests-file", TESTS_FILE)
        out = _pop_flag(args, "--out", IMPORTANCE_FILE)
        n_trees = _pop_flag(args, "--n-trees", None)
        threshold = _pop_flag(args, "--threshold", None)
        kw = dict(repeats=int(_pop_flag(args, "--repeats", "5")),
                  seed=int(_pop_flag(args, "--seed", "0")),
                  threshold=None if threshold is None else float(threshold),
                  backend=_pop_flag(args, "--backend", "auto"))
        if leave_out:
            res = holdout_importance(
                keys, tests_file=tests_file, out_file=out,
                n_trees=int(n_trees) if n_trees else None, **kw)
        else:
            from .engine.detector import Detector
            res = write_importance(Detector.load(detector_file),
                                   tests_file=tests_file, out_file=out, **kw)
        fmt = lambda v: "n/a" if v is None else f"{v:.4f}"
        drops = [(name, entry["f1_drop_mean"])
                 for name, entry in res["importance"].items()]
        # largest first, undefined last; ties keep the groups' order
        drops.sort(key=lambda d: (d[1] is None, -(d[1] or 0.0)))
        top = ", ".join(f"{name} {fmt(v)}" for name, v in drops[:3])
        print(f"wrote {out} ({len(res['importance'])} groups x "
              f"{res['repeats']} repeats, {res['rule']} rule"
              f"{', leave-one-project-out' if leave_out else ''}; "
              f"baseline F1 {fmt(res['baseline']['total'][5])}; "
              f"largest mean F1 drop: {top})")
    elif command == "similar":
        from .constants import DETECTOR_FILE, SIMILAR_FILE, TESTS_FILE
        from .engine.detector import Detector
        from .engine.similar import MAX_K, write_similar
        detector_file = _pop_flag(args, "--detector", DETECTOR_FILE)
        tests_file = _pop_flag(args, "--tests-file", TESTS_FILE)
        corpus = _pop_flag(args, "--corpus", TESTS_FILE)
        out = _pop_flag(args, "--out", SIMILAR_FILE)
        k = int(_pop_flag(args, "--k", "5"))
        if not 1 <= k <= MAX_K:
            raise ValueError(f"--k takes 1..{MAX_K}")
        flaky_only = _pop_flag(args, "--flaky-only", False, boolean=True)
        keep_self = _pop_flag(args, "--keep-self", False, boolean=True)
        backend = _pop_flag(args, "--backend", "auto")
        res = write_similar(Detector.load(detector_file),
                            tests_file=tests_file, corpus=corpus,
                            out_file=out, k=k, flaky_only=flaky_only,
                            skip_self=not keep_self, backend=backend)
        first = res["idx"][:, 0]
        flagged = (res["pred"] == 1) & (first >= 0)
        n_flagged = int((res["pred"] == 1).sum())
        hits = int(res["corpus_labels"][first[flagged]].sum())
        share = "n/a" if n_flagged == 0 else f"{hits / n_flagged:.4f}"
        print(f"wrote {out} ({len(res['pred'])} tests against "
              f"{res['n_candidates']} corpus tests, k {res['k']}; "
              f"{n_flagged} predicted flaky, first neighbour labelled "
              f"flaky for {share} of them)")
    elif command == "dependence":
        from .constants import DEPENDENCE_FILE, DETECTOR_FILE, TESTS_FILE
        from .engine.dependence import write_dependence
        from .engine.detector import Detector
        detector_file = _pop_flag(args, "--detector", DETECTOR_FILE)
        tests_file = _pop_flag(args, "--tests-file", TESTS_FILE)
        out = _pop_flag(args, "--out", DEPENDENCE_FILE)
        grid = int(_pop_flag(args, "--grid", "20"))
        threshold = _pop_flag(args, "--threshold", None)
        ice_out = _pop_flag(args, "--ice-out", None)
        backend = _pop_flag(args, "--backend", "auto")
        res = write_dependence(
            Detector.load(detector_file), tests_file=tests_file,
            out_file=out, ice_out=ice_out, grid=grid,
            threshold=None if threshold is None else float(threshold),
            backend=backend)
        # largest first; ties keep the features' order
        spans = sorted(((name, entry["range"])
                        for name, entry in res["features"].items()),
                       key=lambda s: -s[1])
        top = ", ".join(f"{name} {v:.4f}" for name, v in spans[:3])
        n_jobs = sum(len(e["grid"]) for e in res["features"].values())
        print(f"wrote {out} ({res['n_tests']} tests, "
              f"{len(res['features'])} features, {n_jobs} grid values, "
              f"{res['rule']} rule; baseline mean probability "
              f"{res['baseline']['mean_proba']:.4f}; "
              f"largest range of the mean probability: {top})")
    elif command == "figures":
        offline = _pop_flag(args, "--offline", False, boolean=True)
        from .report.figures import write_figures
        write_figures(offline=offline)
    elif command == "synthetic":
        n_tests = int(_pop_flag(args, "--n-tests", "10000"))
        seed = int(_pop_flag(args, "--seed", "0"))
        from .constants import TESTS_FILE
        from .dataset.synthetic import write_synthetic_tests
        write_synthetic_tests(TESTS_FILE, n_tests=n_tests, seed=seed)
        print(f"wrote {TESTS_FILE} ({n_tests} synthetic tests, seed {seed})")
    else:
        raise ValueError("Unrecognized command given")


if __name__ == "__main__":
    main()
