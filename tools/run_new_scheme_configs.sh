#!/bin/bash
# GPU box: one reference config of each of the cluster.svd / cluster.eig / mnist.svd / zinc_full.svd / zinc_full.eig schemes
# (tests/golden/schemes/: the reference's files, keys as shipped) on synthetic graphs: 2 epochs of training, then the evaluation
# report.  Three keys are changed for the box, in a copy under runs/ (git-ignored): num_epochs 2, distributed false (one process),
# save_path under runs/.
set -e
mkdir -p runs/new_schemes
for rel in cluster/100k/egt.json cluster/100k/egt_epe.json mnist/100k/egt_spe.json zinc_full/500k/egt_spe_do.json zinc_full/500k/egt_epe.json; do
  tag=$(echo "${rel%.json}" | tr / _)
  cfg=runs/new_schemes/$tag.json
  python - "$rel" "$tag" "$cfg" <<'PY'
import json, sys
rel, tag, out = sys.argv[1:]
c = json.load(open("tests/golden/schemes/" + rel))
c.update(num_epochs=2, distributed=False, save_path="runs/new_schemes/" + tag)
json.dump(c, open(out, "w"), indent="\t")
PY
  echo "== $rel"
  python -m egt_amd.training $cfg --synthetic 256 2>&1 | grep -E "CHECKPOINT|DONE|Error|error" | tail -4
  python -m egt_amd.training $cfg --synthetic 256 --evaluate 2>&1 | grep -E "MAE|ccuracy|Recall|crossentropy|LOADED" | tail -14
done
