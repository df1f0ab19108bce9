#!/bin/bash
# GPU box: the reference's five width-64 EGT-Simple configs (configs/ablation/egt_simple: pattern/500k/egt_simple{,_spe,_epe},
# cifar10/100k/egt_simple{,_spe}), keys as shipped, on synthetic graphs: 2 epochs of training each.  tests/golden/egt_simple/
# holds their key/value DATA with the same three keys changed as tests/configs/: num_epochs 2, distributed false (one
# process), save_path under runs/ (git-ignored).
set -e
for cfg in tests/golden/egt_simple/*.json; do
  echo "== $cfg"
  python -m egt_amd.training $cfg --synthetic 256 2>&1 | grep -E "CHECKPOINT|DONE|Error|error" | tail -4
done
