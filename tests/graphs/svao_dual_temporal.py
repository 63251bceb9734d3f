# SVAO with primaryDepthMode DualDepth, its second depth layer chosen by a Switch between TemporalDepthPeel
# (selected, i0) and the DepthPeeling chain (i1): the depth2 data path of the reference's scripts/SVAO_depth.py
# (DepthSelect: 'i0': 'Temporal', 'i1': 'Peel'), in its scripting style.  Loaded by tests/test_temporal_peel.py
# (planned) and tests/test_gpu_temporal_peel.py (executed) with rsd.graph.load_script.
from falcor import *

def render_graph_svao_dual_temporal():
    g = RenderGraph('SVAODualTemporal')
    g.create_pass('GuardBand', 'GuardBand', {'guardBand': 16})
    g.create_pass('GBufferRaster', 'GBufferRaster', {'outputSize': 'Default', 'samplePattern': 'Center', 'forceCullMode': False, 'cull': 'Back'})
    g.create_pass('LinearizeDepth', 'LinearizeDepth', {'depthFormat': 'R32Float'})
    g.create_pass('TemporalDepthPeel', 'TemporalDepthPeel', {'minSeparationDistance': 0.5})
    g.create_pass('DepthPeeling', 'DepthPeeling', {'cullMode': 'Back', 'depthFormat': 'D32Float', 'minSeparationDistance': 0.5})
    g.create_pass('LinearizeDepth2Ref', 'LinearizeDepth', {'depthFormat': 'R32Float'})
    g.create_pass('DepthSelect', 'Switch', {'count': 2, 'selected': 0, 'i0': 'Temporal', 'i1': 'Peel'})
    g.create_pass('CompressNormals', 'CompressNormals', {'viewSpace': True, 'use16Bit': True})
    g.create_pass('SVAO', 'SVAO', {'radius': 1.0, 'primaryDepthMode': 'DualDepth', 'secondaryDepthMode': 'StochasticDepth', 'exponent': 2.0, 'thickness': 0.0, 'stochMapDivisor': 2, 'dualAO': False, 'alphaTest': True, 'stochGuardBand': 64})
    g.add_edge('GuardBand', 'GBufferRaster')
    g.add_edge('GBufferRaster.depth', 'LinearizeDepth.depth')
    g.add_edge('GBufferRaster.depth', 'SVAO.gbufferDepth')
    g.add_edge('GBufferRaster.faceNormalW', 'CompressNormals.normalW')
    g.add_edge('GBufferRaster.mvec', 'TemporalDepthPeel.mvec')
    g.add_edge('LinearizeDepth.linearDepth', 'TemporalDepthPeel.linearZ')
    g.add_edge('LinearizeDepth.linearDepth', 'DepthPeeling.linearZ')
    g.add_edge('DepthPeeling.depth2', 'LinearizeDepth2Ref.depth')
    g.add_edge('TemporalDepthPeel.depth2', 'DepthSelect.i0')
    g.add_edge('LinearizeDepth2Ref.linearDepth', 'DepthSelect.i1')
    g.add_edge('LinearizeDepth.linearDepth', 'SVAO.depth')
    g.add_edge('DepthSelect.out', 'SVAO.depth2')
    g.add_edge('CompressNormals.normalOut', 'SVAO.normals')
    g.mark_output('SVAO.ao')
    g.mark_output('TemporalDepthPeel.depth2')
    g.mark_output('DepthSelect.out')
    g.mark_output('LinearizeDepth2Ref.linearDepth')
    g.mark_output('LinearizeDepth.linearDepth')
    g.mark_output('CompressNormals.normalOut')
    return g

SVAODualTemporal = render_graph_svao_dual_temporal()
try: m.addGraph(SVAODualTemporal)
except NameError: None
