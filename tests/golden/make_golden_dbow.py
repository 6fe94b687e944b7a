#!/usr/bin/env python3
"""Generate tests/golden/dbow/k6_L3.txt and k6_L3.npz (a directory of their own: the extraction tests read every
tests/golden/*.npz as an extraction fixture): a vocabulary the reference's own DBoW2 trained (create() with a
fixed seed, k = 6, L = 3, TF_IDF, L1_NORM, written by saveToTextFile) on oracle-extracted descriptors of synthetic textures,
and what the reference computes with it (LOAD, TRANSFORM and SCORE of oracle/ref/ref_dbow.cc) for a fixed feature set.  Small
training sets give the unbalanced trees k-means really produces.  Needs oracle/_ref/ref_dbow (build() makes it where the
reference tree is present); the tests that read the two files need neither.
Run from the repo root:  python tests/golden/make_golden_dbow.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: F401  (registers my_slam_amd)
import oracle_lib as O
import ref_dbow as D
import my_slam_amd.synth as synth

SEED, K, L, WEIGHTING, SCORING = 7, 6, 3, 0, 0
TRAIN_SEEDS = (21, 22, 23, 24, 25, 26)      # one "image" each, ~60 descriptors
QUERY_SEEDS = (31, 32)
LEVELSUP = (0, 1, 2, 3, 4)


def descriptors(seed, n):
    _, desc, _ = O.Extractor(n).extract(synth.texture(seed, 256, 192))
    return desc


def main():
    train = [descriptors(s, 30) for s in TRAIN_SEEDS]
    os.makedirs(os.path.join(HERE, "dbow"), exist_ok=True)
    txt = os.path.join(HERE, "dbow", "k6_L3.txt")
    with tempfile.TemporaryDirectory() as d:
        (text,) = D.run([D.req_create(SEED, K, L, WEIGHTING, SCORING, train, os.path.join(d, "voc.txt"))])
    with open(txt, "wb") as f:
        f.write(text)
    feats = [descriptors(s, 150) for s in QUERY_SEEDS]
    runs = [(feats[0], l) for l in LEVELSUP] + [(feats[1], 2), (feats[1][:5], 2), (train[0], 1)]
    res = D.run([D.req_load(txt)] + [D.req_transform(f, l) for f, l in runs])
    load, tr = res[0], res[1:]
    pairs = np.array([(a, b) for a in range(len(runs)) for b in range(a, len(runs)) if a in (0, 5, 6, 7) or a == b], np.int32)
    scores = D.run([D.req_load(txt), D.req_score([(tr[a]["bow"], tr[b]["bow"]) for a, b in pairs])])[1]
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt) for x in xs]) if xs else np.zeros(0, dt)
    offs = lambda ns: np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    fv_lists = [idx for t in tr for _, idx in t["fv"]]
    np.savez_compressed(
        os.path.join(HERE, "dbow", "k6_L3.npz"), seed=SEED, train_sizes=np.array([len(t) for t in train]),
        features=cat([f for f, _ in runs], np.uint8).reshape(-1, 32), levelsup=np.array([l for _, l in runs], np.int32),
        run_off=offs([len(f) for f, _ in runs]),
        word=cat([t["word"] for t in tr], np.uint32), weight=cat([t["weight"] for t in tr], np.float64),
        node=cat([t["node"] for t in tr], np.uint32),
        bow_off=offs([len(t["bow"][0]) for t in tr]), bow_ids=cat([t["bow"][0] for t in tr], np.int32),
        bow_vals=cat([t["bow"][1] for t in tr], np.float64),
        fv_off=offs([len(t["fv"]) for t in tr]), fv_node=cat([[nid for nid, _ in t["fv"]] for t in tr], np.uint32),
        fv_idx_off=offs([len(x) for x in fv_lists]), fv_idx=cat(fv_lists, np.int32),
        score_pairs=pairs, scores=scores, **{"load_" + k: v for k, v in load.items()})
    print("nodes %d, words %d, %d bytes of text; %d runs, %d scores" % (load["nnodes"], load["nwords"], len(text), len(runs), len(scores)))


if __name__ == "__main__":
    main()
