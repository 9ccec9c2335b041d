"""Drop-in for EDT_EVOMERGE/train/crossover.py: SLERP crossover of two 7B-class causal LMs (bf16)
on a worker, driven by EDT_EVOMERGE/edt.py:262-280 through the CLI

    python -m evolutionarydistributedtraining_amd.evomerge_crossover --model1_path A --model2_path B --output_path O

The reference moves each tensor to the GPU and back and SLERPs it in numpy (its LazyTensorLoader,
EDT_EVOMERGE/train/crossover.py:86-146); here both bodies are merged in HBM in one multi-tensor
pass and the bf16 result becomes model_1's body (the reference's `model_merged.model.load_state_dict`,
:142, rounds the fp32 SLERP to bf16 the same way): written to a fresh buffer in the single-pass form
and model_1's parameters re-pointed at it (merge.slerp_into_module_), since writing into model_1's
own tensors — the parent being read — would force the two-pass form.
"""
from __future__ import annotations

import json
import os

import torch

from .merge import (LazyTensorLoader, interpolate_t, lerp, maybe_torch, merge_models_into_, merge_plan,  # noqa: F401
                    normalize, slerp, slerp_state_dicts, task_merge_models_into_, uniform_dna_crossover)

__all__ = ["slerp", "lerp", "interpolate_t", "load_model_from_path", "run_slerp_merge_from_config",
           "run_linear_merge_5050", "crossover_main", "uniform_dna_crossover", "SELF_ATTN_T_CURVE",
           "MLP_T_CURVE", "LazyTensorLoader", "maybe_torch", "normalize", "task_merge_config",
           "run_task_merge_from_config", "task_merge_main"]

SELF_ATTN_T_CURVE = [0, 0.5, 0.3, 0.7, 1]      # EDT_EVOMERGE/train/crossover.py:174-175
MLP_T_CURVE = [1, 0.5, 0.7, 0.3, 0]


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def load_model_from_path(folder_path: str):
    """bf16 AutoModelForCausalLM on the GPU (EDT_EVOMERGE/train/crossover.py:66-69)."""
    from transformers import AutoConfig, AutoModelForCausalLM
    config = AutoConfig.from_pretrained(folder_path, trust_remote_code=True, cache_dir="cache")
    model = AutoModelForCausalLM.from_pretrained(folder_path, config=config, torch_dtype=torch.bfloat16,
                                                 trust_remote_code=True, cache_dir="cache")
    return model.to(_device())


def run_slerp_merge_from_config(merge_config_dict: dict, model_1, model_2, config_1, config_2,
                                merge_output_path: str, base_model, device=None) -> str:
    """SLERP model_1 / model_2 (bodies, `.model`) into base_model.model and save base_model
    (EDT_EVOMERGE/train/crossover.py:104-146). `device` picks the GPU (None: current)."""
    num_layers = min(config_1.num_hidden_layers, config_2.num_hidden_layers)
    # the merge lands in the target's parameters (== load_state_dict of the merged dict). The target
    # may be model_1 itself (the reference passes base_model=model_1): then the children go to a
    # fresh buffer in one pass and the parameters are re-pointed at it (merge.slerp_into_module_)
    merge_models_into_(base_model.model, model_1, model_2, merge_config_dict, num_layers, device=device)
    base_model.save_pretrained(merge_output_path)
    print("SLERP merging complete! Model saved at:", merge_output_path)
    return merge_output_path


def run_linear_merge_5050(model_1, model_2, config_1, config_2, merge_output_path: str) -> str:
    """t = 0.5 lerp of every state-dict tensor into AutoModel.from_config, saved
    (EDT_EVOMERGE/train/crossover.py:149-163)."""
    from transformers import AutoModel
    merged_model = AutoModel.from_config(model_1.config, trust_remote_code=True)
    sd1, sd2 = model_1.state_dict(), model_2.state_dict()
    merged = {k: lerp(0.5, sd1[k], sd2[k]) for k in sd1.keys()}
    merged_model.load_state_dict(merged)
    merged_model.save_pretrained(merge_output_path)
    print("Linear 50-50 merging complete! Model saved at:", merge_output_path)
    return merge_output_path


def slerp_config(model1_path: str, model2_path: str, num_layers: int) -> dict:
    return {
        "slices": [{"sources": [{"model": model1_path, "layer_range": [0, num_layers]},
                                {"model": model2_path, "layer_range": [0, num_layers]}]}],
        "merge_method": "slerp", "base_model": model1_path,
        "parameters": {"t": [{"filter": "self_attn", "value": SELF_ATTN_T_CURVE},
                             {"filter": "mlp", "value": MLP_T_CURVE}, {"value": 0.5}]},
        "dtype": "float32", "tokenizer_source": None,
    }


def task_merge_config(base_path: str, model_paths, merge_method: str = "dare_ties", weight=1.0, density=1.0,
                      normalize: bool = True, lam: float = 1.0) -> dict:
    """A MergeKit-style config of a task-vector merge of the models at model_paths relative to the one
    at base_path: merge_method task_arithmetic, dare_linear or dare_ties; weight / density a scalar
    for every model or one per model (each a scalar or a [{filter, value}] list, routed per key as
    SLERP's t is)."""
    def per_model(v, i):
        return v[i] if isinstance(v, (list, tuple)) and len(v) == len(model_paths) and not any(
            isinstance(p, dict) for p in v) else v
    return {
        "merge_method": merge_method, "base_model": base_path,
        "models": [{"model": base_path}] + [{"model": p, "parameters": {"weight": per_model(weight, i),
                                                                         "density": per_model(density, i)}}
                                             for i, p in enumerate(model_paths)],
        "parameters": {"normalize": normalize, "lambda": lam},
        "dtype": "bfloat16", "tokenizer_source": None,
    }


def run_task_merge_from_config(merge_config_dict: dict, base_body, model_bodies, configs, merge_output_path: str,
                               base_model, seed: int = 0, step: int = 0, device=None) -> str:
    """Merge the fine-tuned bodies (`.model` of each causal LM) relative to base_body into
    base_model.model by the config's task-vector method, one fused pass over the K + 1 bodies where they
    lie in HBM (merge.task_merge_models_into_; base_model.model is usually base_body: in place), and
    save base_model. configs: the models' configs (the merge covers min(num_hidden_layers) layers)."""
    num_layers = min(c.num_hidden_layers for c in configs)
    task_merge_models_into_(base_model.model, base_body, list(model_bodies), merge_config_dict, num_layers, seed=seed,
                            step=step, device=device)
    base_model.save_pretrained(merge_output_path)
    print(f"{merge_config_dict['merge_method']} merging complete! Model saved at:", merge_output_path)
    return merge_output_path


def task_merge_main(base_path: str, model_paths, output_path: str, merge_method: str = "dare_ties", weight=1.0,
                    density=1.0, seed: int = 0) -> None:
    """Child of K fine-tuned models of one base: the task-vector merge into the base, tokenizer saved."""
    from transformers import AutoTokenizer
    base = load_model_from_path(base_path)
    models = [load_model_from_path(p) for p in model_paths]
    cfg = task_merge_config(base_path, list(model_paths), merge_method, weight, density)
    AutoTokenizer.from_pretrained(base_path, trust_remote_code=True, cache_dir="cache").save_pretrained(output_path)
    run_task_merge_from_config(cfg, base.model, [m.model for m in models], [base.config] + [m.config for m in models],
                               output_path, base_model=base, seed=seed)
    print("Done!")


def crossover_main(model1_path: str, model2_path: str, output_path: str) -> None:
    """Child of two parents: SLERP into parent 1, tokenizer, genome.json
    (EDT_EVOMERGE/train/crossover.py:166-229)."""
    from transformers import AutoTokenizer
    model_1 = load_model_from_path(model1_path)
    model_2 = load_model_from_path(model2_path)
    num_layers = min(model_1.config.num_hidden_layers, model_2.config.num_hidden_layers)
    cfg = slerp_config(model1_path, model2_path, num_layers)
    tokenizer = AutoTokenizer.from_pretrained(model1_path, trust_remote_code=True, cache_dir="cache")
    tokenizer.save_pretrained(output_path)
    run_slerp_merge_from_config(cfg, model_1.model, model_2.model, model_1.config, model_2.config,
                                output_path, base_model=model_1)
    with open(os.path.join(model1_path, "genome.json")) as f:
        p1 = json.load(f)
    with open(os.path.join(model2_path, "genome.json")) as f:
        p2 = json.load(f)
    for g in (p1, p2):
        g.pop("p1", None)
        g.pop("p2", None)
    genome = {"fitness": 0.0, "model_path": output_path,
              "dna": uniform_dna_crossover(p1["dna"], p2["dna"]), "p1": p1, "p2": p2}
    with open(os.path.join(output_path, "genome.json"), "w") as f:
        json.dump(genome, f, indent=4)
    print("Done!")


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="SLERP merge two Hugging Face models, or task-vector merge K "
                                             "fine-tuned models of one base (MI355X).")
    ap.add_argument("--model1_path", type=str)
    ap.add_argument("--model2_path", type=str)
    ap.add_argument("--output_path", type=str, default="crossover_result")
    ap.add_argument("--merge_method", type=str, default=None, choices=["slerp", "task_arithmetic", "dare_linear",
                                                                       "dare_ties"])
    ap.add_argument("--base_path", type=str, default=None)
    ap.add_argument("--model_path", type=str, action="append", default=None, help="repeat: one per fine-tuned model")
    ap.add_argument("--weight", type=float, action="append", default=None, help="one for all models, or one per model")
    ap.add_argument("--density", type=float, action="append", default=None, help="one for all models, or one per model")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    if a.merge_method in (None, "slerp"):
        if any(v is not None for v in (a.base_path, a.model_path, a.weight, a.density)):
            ap.error("--base_path, --model_path, --weight and --density belong to a task-vector --merge_method")
        if not a.model1_path or not a.model2_path:
            ap.error("the following arguments are required: --model1_path, --model2_path")
        crossover_main(a.model1_path, a.model2_path, a.output_path)
        return
    if not a.base_path or not a.model_path:
        ap.error(f"--merge_method {a.merge_method} needs --base_path and at least one --model_path")

    def per_model(v):
        if v is None or len(v) == 1:
            return 1.0 if v is None else v[0]
        if len(v) != len(a.model_path):
            ap.error("--weight / --density: one value, or one per --model_path")
        return v
    task_merge_main(a.base_path, a.model_path, a.output_path, a.merge_method, per_model(a.weight), per_model(a.density),
                    a.seed)


if __name__ == "__main__":
    main()
