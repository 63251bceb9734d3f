# SVAO with primaryDepthMode DualDepth, its second depth layer produced by DepthPeeling: the
# depth chain of the reference's SVAO graphs (LinearizeDepth -> DepthPeeling -> LinearizeDepth0 ->
# SVAO.depth2), in their scripting style.  Loaded by tests/test_depth_peel.py (planned) and
# tests/test_gpu_depth_peel.py (executed) with rsd.graph.load_script.
from falcor import *

def render_graph_svao_dual_peel():
    g = RenderGraph('SVAODualPeel')
    g.create_pass('GuardBand', 'GuardBand', {'guardBand': 8})
    g.create_pass('GBufferRaster', 'GBufferRaster', {'outputSize': 'Default', 'samplePattern': 'Center', 'forceCullMode': False, 'cull': 'Back'})
    g.create_pass('LinearizeDepth', 'LinearizeDepth', {'depthFormat': 'R32Float'})
    g.create_pass('DepthPeeling', 'DepthPeeling', {'cullMode': 'Back', 'depthFormat': 'D32Float', 'minSeparationDistance': 0.5})
    g.create_pass('LinearizeDepth0', 'LinearizeDepth', {'depthFormat': 'R32Float'})
    g.create_pass('CompressNormals', 'CompressNormals', {'viewSpace': True, 'use16Bit': True})
    g.create_pass('SVAO', 'SVAO', {'radius': 2.0, 'primaryDepthMode': 'DualDepth', 'secondaryDepthMode': 'StochasticDepth', 'exponent': 2.0, 'thickness': 0.0, 'stochMapDivisor': 1, 'dualAO': False, 'alphaTest': True, 'stochGuardBand': 16})
    g.add_edge('GuardBand', 'GBufferRaster')
    g.add_edge('GBufferRaster.depth', 'LinearizeDepth.depth')
    g.add_edge('GBufferRaster.depth', 'SVAO.gbufferDepth')
    g.add_edge('GBufferRaster.faceNormalW', 'CompressNormals.normalW')
    g.add_edge('LinearizeDepth.linearDepth', 'DepthPeeling.linearZ')
    g.add_edge('DepthPeeling.depth2', 'LinearizeDepth0.depth')
    g.add_edge('LinearizeDepth.linearDepth', 'SVAO.depth')
    g.add_edge('LinearizeDepth0.linearDepth', 'SVAO.depth2')
    g.add_edge('CompressNormals.normalOut', 'SVAO.normals')
    g.mark_output('SVAO.ao')
    return g

SVAODualPeel = render_graph_svao_dual_peel()
try: m.addGraph(SVAODualPeel)
except NameError: None
