#!/usr/bin/env python
"""Export the environment light a checkpoint has learned as a lat-long panorama: env_light.hdr (linear radiance, Radiance RGBE -- the input of
the reference's relight.py --hdr) and env_light.png (gamma-mapped, clipped to [0, 1]) through nero_amd.envlight.

    python scripts/extract_env_light.py --cfg configs/material/syn/bell.yaml --model data/model/bell_material/model.pth --out data/env/bell
    python scripts/extract_env_light.py --stage 1 --cfg configs/shape/syn/bell.yaml --model data/model/bell_shape/model.pth --roughness 0.3 --out out_dir

--stage 2 (default): NeROMaterialRenderer.env_light, the reference's MCShadingNetwork.env_light.  --stage 1: the same panorama from the
Stage-I AppShadingNetwork.outer_light; --roughness above 0 gives the light pre-filtered for that roughness.  --cfg: the YAML (or JSON) of the
stage; --model: a trainer checkpoint (its `network_state_dict` entry) or a bare state dict; without it the maps show the freshly initialised
network (a dry run).  The Stage-II light does not depend on the mesh: --mesh or the cfg's `mesh` entry is used when the file exists, else a
stand-in icosphere.  Row 0 of both files is the pole el = +pi / 2 (up: +z for `real` databases, +y otherwise), columns run from az = 3 pi / 2
down to -pi / 2."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_cfg(path):
    text = open(path).read()
    if path.endswith('.json'):
        return json.loads(text)
    import yaml
    return yaml.safe_load(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--cfg')
    ap.add_argument('--model', '--ckpt', dest='model')
    ap.add_argument('--stage', type=int, default=2, choices=(1, 2))
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--roughness', type=float, default=0.0, help='Stage I only: the roughness the light is pre-filtered for')
    ap.add_argument('--mesh', help='Stage II only: PLY of the Stage-I mesh (the light does not depend on it)')
    ap.add_argument('--chunk', type=int, default=None)
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    if args.stage == 2 and args.roughness != 0.0:
        ap.error('--roughness applies to --stage 1: the Stage-II light is encoded at roughness 0 (network/field.py:1049-1055)')
    from nero_amd import envlight as E
    from nero_amd.metrics import color_map_backward
    from nero_amd.renderer import NeROMaterialRenderer, NeROShapeRenderer
    from nero_amd.texture import write_png
    cfg = load_cfg(args.cfg) if args.cfg else {}
    if args.stage == 1:
        net = NeROShapeRenderer({k: v for k, v in cfg.items() if k in NeROShapeRenderer.default_cfg}, training=False)
    else:
        mesh_path = args.mesh or cfg.get('mesh')
        if mesh_path and os.path.exists(mesh_path):
            from nero_amd.mesh import read_ply
            mesh = read_ply(mesh_path)
        else:
            from nero_amd.synthetic import icosphere
            mesh = icosphere(1, 0.5)
        net = NeROMaterialRenderer({k: cfg[k] for k in ('shader_cfg', 'database_name') if k in cfg}, is_train=False, mesh=mesh)
    if args.model:
        sd = torch.load(args.model, map_location='cpu')
        net.load_state_dict(sd.get('network_state_dict', sd))
    else:
        print('no --model: exporting the light of the freshly initialised network', file=sys.stderr)
    net = net.cuda().eval()
    kw = dict(chunk=args.chunk)
    if args.stage == 1:
        kw['roughness'] = args.roughness
    lin = net.env_light(args.height, args.width, gamma=False, **kw)
    gam = net.env_light(args.height, args.width, gamma=True, **kw)
    os.makedirs(args.out, exist_ok=True)
    hdr, png = os.path.join(args.out, 'env_light.hdr'), os.path.join(args.out, 'env_light.png')
    E.write_hdr(hdr, lin)
    write_png(png, color_map_backward(gam))
    print(json.dumps({'hdr': hdr, 'png': png, 'stage': args.stage, 'height': args.height, 'width': args.width, 'roughness': args.roughness,
                      'min': float(lin.min()), 'max': float(lin.max())}))


if __name__ == '__main__':
    main()
