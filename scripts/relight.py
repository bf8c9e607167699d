"""Relight a Stage-I mesh with its Stage-II materials under an HDR environment map, on the GPU: the reference's relight.py without Blender
(nero_amd.relight; direct lighting with shadows, and with --bounces 1 one inter-reflection -- DESIGN.md 9.12, 9.12.2).

    python scripts/relight.py --mesh M.ply --material DIR --hdr E.hdr --name N
    python scripts/relight.py --mesh M.ply --cfg configs/material/x.yaml --model model.pth --hdr E.hdr --name N
    python scripts/relight.py --mesh mesh_0.obj --textured --hdr E.hdr --name N

--textured: --mesh is the textured OBJ extract_texture_maps.py wrote, with its MTL and the albedo / metallic / roughness maps beside it; the
materials are read from the maps at every hit, filtered to the pixel's footprint; --lod-bias B shifts the level of detail
(+1: one level blurrier).  When the asset has a normal map (extract_texture_maps.py --normal-map) it perturbs the shading normal at every hit
 and --normals defaults to the frame the map was baked in; --no-normal-map ignores it.  --material DIR holds metallic.npy, roughness.npy, albedo.npy as extract_materials.py writes them (per vertex of --mesh); with --cfg/--model the
materials are predicted from the trained Stage-II network instead.  --normals angle (or area) shades with smooth vertex normals computed
from the mesh instead of flat face normals.  --denoise filters the picture's signals with the edge-aware denoiser
(DESIGN.md 9.12.3).  Writes <out>/<name>/<k>.png, RGBA, one per view of the reference's orbit."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--mesh', required=True)
    ap.add_argument('--material', help='directory with metallic.npy, roughness.npy, albedo.npy')
    ap.add_argument('--cfg', help='Stage-II yaml config (with --model), instead of --material')
    ap.add_argument('--model', help='Stage-II checkpoint')
    ap.add_argument('--hdr', required=True)
    ap.add_argument('--name', required=True)
    ap.add_argument('--trans', action='store_true', help="the reference's 90 degree turn about x, applied to the vertices")
    ap.add_argument('--width', type=int, default=800)
    ap.add_argument('--height', type=int, default=800)
    ap.add_argument('--samples', type=int, nargs='+', default=[128, 128], help='diffuse and specular directions per pixel (one number: both); a third number adds that many '
                         'directions drawn from the map itself, all three combined by multiple importance sampling -- the same picture with far '
                         'less noise under a map with a sun or a lamp in it, and no need for --clamp')
    ap.add_argument('--num', type=int, default=360)
    ap.add_argument('--azimuth', type=float, default=0.0)
    ap.add_argument('--elevation', type=float, default=30.0)
    ap.add_argument('--cam_dist', type=float, default=3.0)
    ap.add_argument('--ssaa', type=int, default=1)
    ap.add_argument('--clamp', type=float, default=None, help="cap on the environment's radiance per channel (firefly control)")
    ap.add_argument('--convention', default='blender', choices=['blender', 'nero', 'nero_real'],
                    help="how the map is laid out: Blender's equirectangular image, or this project's env_light grid (is_real 0 / 1)")
    ap.add_argument('--bounces', type=int, default=0, choices=[0, 1],
                    help='1: a direction that meets the mesh fetches the light that surface sends back (one inter-reflection) instead of black')
    ap.add_argument('--normals', default=None, choices=['flat', 'angle', 'area'],
                    help='flat (the default): face normals; angle / area: smooth vertex normals computed from the mesh, face normals weighted by angle '
                         "or by area.  With a textured asset that has a normal map the default is the frame the map records")
    ap.add_argument('--no-normal-map', action='store_true', help="--textured: ignore the asset's normal map")
    ap.add_argument('--denoise', action='store_true',
                    help='filter the diffuse, specular and indirect signals with the edge-aware denoiser before they are summed (DESIGN.md 9.12.3): '
                         'fewer --samples for the same noise')
    ap.add_argument('--denoise-iterations', type=int, default=None, metavar='N', help='a-trous passes of --denoise (default 5), the stride doubling from 1')
    ap.add_argument('--denoise-sigma', type=float, default=None, metavar='L',
                    help='--denoise: how many standard deviations of luminance a tap may differ by (default 4)')
    ap.add_argument('--textured', action='store_true',
                    help='--mesh is a textured OBJ (write_textured_obj): read the materials from its maps instead of --material / --cfg and --model')
    ap.add_argument('--lod-bias', type=float, default=None, metavar='B', help='--textured: levels added to the level of detail (default 0)')
    ap.add_argument('--out', default='data/relight')
    a = ap.parse_args(argv)
    if a.lod_bias is not None and not a.textured:
        ap.error('--lod-bias needs --textured')
    if a.no_normal_map and not a.textured:
        ap.error('--no-normal-map needs --textured')
    if a.textured and (a.material or a.cfg or a.model):
        ap.error('--textured reads the materials from the maps: give no --material, --cfg or --model')
    denoise = None
    if a.denoise:
        denoise = {k: v for k, v in (('iterations', a.denoise_iterations), ('sigma_l', a.denoise_sigma)) if v is not None} or True
    elif a.denoise_iterations is not None or a.denoise_sigma is not None:
        ap.error('--denoise-iterations and --denoise-sigma need --denoise')

    import torch
    from nero_amd.mesh import read_ply
    from nero_amd.relight import Relighter, load_materials
    textures, materials = None, None
    if a.textured:
        from nero_amd.texture import read_textured_obj
        textures = read_textured_obj(a.mesh)
        if not all(k in textures for k in ('albedo', 'metallic', 'roughness')):
            raise SystemExit(f'{a.mesh}: the albedo, metallic and roughness maps its MTL names are not beside it')
        verts, tris = textures['v'], textures['f']
    else:
        verts, tris = read_ply(a.mesh)
    verts = np.asarray(verts, np.float32)
    if a.textured:
        materials = None                                                  # (Relighter fetches them from the maps)
    elif a.material:
        materials = load_materials(a.material)
    elif a.cfg and a.model:
        import yaml
        from nero_amd.renderer import NeROMaterialRenderer
        with open(a.cfg) as fh:
            cfg = yaml.safe_load(fh)
        net = NeROMaterialRenderer(cfg, is_train=False, mesh=(verts, np.asarray(tris, np.int32)))
        ckpt = torch.load(a.model, map_location='cpu')
        net.load_state_dict(ckpt.get('network_state_dict', ckpt))
        net = net.cuda().eval()
        materials = net.predict_materials_of_vertices(torch.from_numpy(verts).cuda())
    else:
        ap.error('give --material DIR, or --cfg and --model')
    if materials is not None and materials['albedo'].shape[0] != verts.shape[0]:
        raise SystemExit(f"{materials['albedo'].shape[0]} material rows for {verts.shape[0]} vertices: --material does not belong to --mesh")
    if a.trans:                                                           # (x, y, z) -> (x, -z, y)
        verts = verts @ np.asarray([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32).T
    if len(a.samples) > 3 or min(a.samples) < 1:
        ap.error('--samples takes one to three positive integers')
    samples = tuple(a.samples) if len(a.samples) == 3 else tuple((a.samples * 2)[:2])
    tex_kw = dict(textures=textures, lod_bias=a.lod_bias or 0.0) if a.textured else {}
    normals = a.normals
    if a.textured and 'normal' in textures and not a.no_normal_map:
        tex_kw['normal_map'] = {'normal': textures['normal'], 'vt': textures['vt'], 'ft': textures['ft'], 'space': textures['normal_space']}
        if normals is None and textures['normal_frame'] in ('angle', 'area'):
            normals = textures['normal_frame']
        elif textures['normal_frame'] not in ('angle', 'area') and textures['normal_space'] == 'tangent':
            # (as Relighter.from_asset: the frame normals of such an asset are not in the file, and --normals cannot stand in for them)
            raise SystemExit(f"{a.mesh}: its tangent-space normal map was baked in the frame of normals the asset does not hold "
                             f"(normals={textures['normal_frame']}): relight it through Relighter.from_asset(..., normals=<those normals>), or pass --no-normal-map")
    rl = Relighter(verts, tris, materials, a.hdr, convention=a.convention, normals=None if normals in (None, 'flat') else normals, **tex_kw)
    out_dir = os.path.join(a.out, a.name)
    paths = rl.render_orbit(out_dir, num=a.num, azimuth=a.azimuth, elevation=a.elevation, dist=a.cam_dist, h=a.height, w=a.width,
                            samples=samples, ssaa=a.ssaa, clamp=a.clamp, bounces=a.bounces, denoise=denoise)
    print(f'{len(paths)} views of {a.width} x {a.height} at {"+".join(str(n) for n in samples)} samples, {a.bounces} bounces -> {out_dir}')


if __name__ == '__main__':
    main()
