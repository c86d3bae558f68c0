"""Generate tests/golden/reference_configs.json: the inference-path keys of the reference's eight configs/*.yaml, parsed by
gomatching_amd.config.setup_cfg (container-only).

TEST INFRASTRUCTURE.  Run in the build container, where /root/reference exists:

    python -m oracle.gen_golden_configs

Only the parsed values are committed (tests/test_host_rules_cpu.py compares the builtin configs against them); no yaml travels.
"""
import json
import os

from gomatching_amd.config import REFERENCE_YAML, setup_cfg
from oracle.ref_shim import REF_ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(os.path.dirname(HERE), "tests", "golden")
KEYS = ["MODEL.ROI_HEADS.NAME", "MODEL.ROI_HEADS.WITH_RESR", "MODEL.TRANSFORMER.NUM_QUERIES", "MODEL.TRANSFORMER.VOC_SIZE",
        "MODEL.TRANSFORMER.INFERENCE_TH_TEST", "INPUT.MIN_SIZE_TEST", "INPUT.MAX_SIZE_TEST", "VIDEO_TEST",
        "MODEL.ASSO_HEAD.ASSO_THRESH_TEST", "MODEL.ASSO_HEAD.NUM_WEIGHT_LAYERS", "MODEL.ASSO_HEAD.NUM_FC",
        "MODEL.ASSO_HEAD.NO_POS_EMB", "INPUT.VIDEO.TEST_LEN", "INPUT.FORMAT"]


def lookup(cfg, key):
    for part in key.split("."):
        cfg = getattr(cfg, part)
    return json.loads(json.dumps(dict(cfg) if isinstance(cfg, dict) else cfg))


def main():
    out = {}
    for name, yaml_name in sorted(REFERENCE_YAML.items()):
        cfg = setup_cfg(os.path.join(REF_ROOT, "configs", yaml_name))
        out[name] = {k: lookup(cfg, k) for k in KEYS}
    path = os.path.join(GOLD, "reference_configs.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
