function [counts, summary, edges] = volumeHistogram(r, nbins, limits, varargin)
% volumeHistogram  Histogram and per-label statistics of the resident volume.
%
%   counts = volumeHistogram(r, 256, [0 1])
%   [counts, summary, edges] = volumeHistogram(r, 256, [0 1], 'Source', 'absorption')
%   [counts, summary] = volumeHistogram(r, 64, [0 1], 'Labels', [3 5])      % labels 3..7 and "other"
%   [counts, summary] = volumeHistogram(r, 64, [0 1], 'UseClip', true)     % inside the ClipPlanes only
%
% What the renderer holds -- a RawVolume widened to single, label gains applied -- not what the host
% array holds (volumeRender('volume_histogram', ...), vr_volume_histogram in include/vrhip.h): the numbers
% an isosurface level, a transfer function's limits or a label gain are chosen from.
%   nbins, limits     nbins equal bins over limits = [lo hi]; a voxel equal to hi falls in the last bin, as
%                     with histcounts.  Voxels below lo, above hi and NaN voxels are counted apart.
%   'Source'          'emission' (default) | 'absorption' | 'reflection'.
%   'Labels'          [first count]: one row per label value first .. first+count-1 (0-based label values
%                     of the label volume, count 1..256) and a last row that collects every other label.
%                     Default: one row over all voxels; the labels are not read.
%   'UseClip'         true: only voxels whose centre the clip planes set on r keep.
% counts is uint64 [nbins rows]: counts(:, k) is row k.  summary is a table with one row per row of the
% histogram: total, below, above, nan, ninf (inf voxels, also counted in below / above), min, max (over
% the non-NaN voxels; NaN without one), sum and mean (over the finite voxels).  edges are the nbins + 1
% bin edges.
%
% Not run under MATLAB by this project's tests (they drive the same mex command through a stand-in of
% the MEX API).
p = inputParser;
addParameter(p, 'Source', 'emission');
addParameter(p, 'Labels', [0 0]);
addParameter(p, 'UseClip', false);
parse(p, varargin{:});
o = p.Results;
if all([islogical(r.VolumeReflection), islogical(r.VolumeAbsorption), islogical(r.VolumeEmission)])
    error('Not all volumes are properly set!');
end
if numel(limits) ~= 2
    error('limits must be [lo hi].');
end
if numel(o.Labels) ~= 2
    error('Labels must be [first count].');
end
r.syncVolumes();
[counts, s] = volumeRender('volume_histogram', r.objectHandle, lower(o.Source), double(nbins), ...
    single(limits(:)'), int32(o.Labels(:)'), logical(o.UseClip));
finite = s(:, 1) - s(:, 4) - s(:, 5);
summary = table(s(:, 1), s(:, 2), s(:, 3), s(:, 4), s(:, 5), single(s(:, 6)), single(s(:, 7)), s(:, 8), ...
    s(:, 8) ./ finite, 'VariableNames', ...
    {'total', 'below', 'above', 'nan', 'ninf', 'min', 'max', 'sum', 'mean'});
edges = double(limits(1)) + (0:double(nbins)) * (double(limits(2)) - double(limits(1))) / double(nbins);
end
